// jpeg_huff.hip — the Huffman coder of the JPEG encoder on the device (contract: include/facehip.h, "JPEG out"): int16 coefficients in
// device memory -> complete baseline JFIF files in a device byte arena, byte for byte fh_jpeg_write's (image_io.cpp, which stays the
// oracle: tests/test_gpu_jpeg_huff.py).  The code tables and the header bytes come from the host writer itself (fh::jpeg_huff_codes,
// fh_jpeg_write_header) in the staged tables; this file restates only the walk over the blocks and encode_block's symbol rule.
//
// A batch is the live images' blocks in SCAN order (MCU by MCU; inside an MCU component by component, v rows of h blocks), image after
// image: B blocks, block g of the batch.  The passes, every one a launch of its own — no kernel waits for another workgroup:
//   huff_size_kernel     one wave per block (eight consecutive blocks in turn), lane = zigzag position.  __ballot of the non-zero lanes
//                        is jchuff.c's bit mask; a non-zero lane finds its run in the mask and forms its whole code — the ZRLs of run >> 4, the symbol (run & 15) << 4 | size,
//                        the value bits: at most 3 * 11 + 16 + 10 = 59 bits, one 64-bit word; lane 0 codes the DC difference against the
//                        DC of the previous block of the same component (the block before it in the MCU, else the component's last block
//                        of the previous MCU, else 0: a load, not a chain), lane 63 the EOB when its coefficient is zero.  A wave prefix sum
//                        of the lengths gives bits[g] (= fh_jpeg_scan_bits).  A size the tables cannot code (DC above 11, AC above 10) is
//                        clamped BEFORE it indexes the table and marks the image as failed.
//   scan (three launches)  off[0 .. B] = the exclusive prefix sum of bits over the batch: per 1024 entries a workgroup sum, one workgroup
//                        over the partial sums (serial per lane over a host-given count), and the apply pass.  Used a second time for the
//                        0xFF counts below.  huff_totals_kernel takes the images' totals as differences at the images' first blocks.
//   — the host reads the images' bit totals and failure flags (FIRST synchronisation), places the unstuffed streams (16-byte aligned,
//     zeroed) and their 1024-byte chunks —
//   huff_pack_kernel     the size pass's codes again, now placed: the block's bits are gathered in LDS at (bit offset & 31), MSB first, and
//                        leave as whole 32-bit words in stream byte order: the first and the last word of a block, which neighbours may
//                        share, by atomic OR into the zeroed stream (OR commutes: the bytes do not depend on timing), the words between
//                        by plain stores.  The last block of an image adds the one-bits that pad the last byte (ByteSink::flush).
//   huff_ff_kernel       0xFF bytes per chunk of FH_JPEG_STUFF_CHUNK = 1024 stream bytes; the scan above; the images' totals.
//   — the host reads the images' 0xFF totals (SECOND synchronisation), sizes the files and lays them back to back in the arena —
//   huff_file_kernel     per chunk: every stream byte to header + index + the 0xFF bytes in front of it, a zero behind every 0xFF; the
//                        image's first chunk copies the header, its last one writes FF D9.  Asynchronous on the stream.
//
// Widths.  A block has at most 11 + 11 + 63 * 26 = 1660 bits (a ZRL replaces sixteen coefficients that would cost more), a scan chunk of
// 1024 blocks below 2^21: uint32.  The call refuses a batch of 2^31 blocks or more on the host, so block indices are 31-bit and every
// offset over the batch is below 2^31 * 1660 < 2^42 bits: the offsets, the partial sums and all byte offsets are 64-bit, and nothing
// narrower ever holds a sum over more than one chunk.  0xFF counts per chunk are at most 1024.  Every loop in a kernel runs over a count
// the host put into the table or the launch (entries of a table, partial sums, header bytes <= kHdrSlot) or is a fixed unrolled one.
#include <hip/hip_runtime.h>

#include <cstring>
#include <stdexcept>
#include <string>

#include "jpeg_enc.h"
#include "kernels.h"

namespace fh {

namespace {

constexpr int kLanes = 256;                          // lanes per workgroup of every kernel here
constexpr int kCodeWaves = kLanes / 64;              // waves per workgroup; in the size and the pack pass a wave takes a block at a time ...
constexpr int kWaveBlocks = 8;                       // ... of this many consecutive blocks of the batch
constexpr int kScanChunk = kLanes * 4;               // entries per workgroup of the scan
constexpr int kStuffChunk = FH_JPEG_STUFF_CHUNK;     // stream bytes per workgroup of the stuffing passes: one dword per lane
constexpr int kHdrSlot = 704;                        // bytes of a header in the files table (SOI .. SOS with three quantiser tables: 692)
constexpr int kBlockWords = 56;                      // LDS words of a block in the pack pass: (31 + 1660 + 7 + 31) / 32 = 54
static_assert(kStuffChunk == kLanes * 4, "one dword of the stream per lane");
static_assert(kBlockWords <= 64, "one lane per word");

// One image of the batch as the size and the pack pass see it (chroma is 1 x 1 in every layout fh_jpeg_enc_check accepts).
struct HuffImg {
    long long coef_base;                             // of the image in d_coef, int16 elements
    long long coef_off[3];
    int32_t wblocks[3];
    int32_t ncomp, h0, v0, mcux, bpm;                // luma sampling factors, MCUs per row, blocks per MCU
};
static_assert(sizeof(HuffImg) % 8 == 0, "the tables behind the rows are int64");

__device__ const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the entry whose run holds g: start[e] <= g < start[e + 1] (empty entries are never hit).  Uniform over the wave.  (A private copy, as
// jpeg_enc.hip's and jpeg_dev.hip's, so that their kernels stay as they are.)
__device__ __forceinline__ int find_entry(const long long* __restrict__ start, int entries, long long g) {
    int lo = 0, hi = entries;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// exclusive prefix sum of v over the workgroup's kLanes lanes and the workgroup's total; sums = kCodeWaves words of LDS
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sums, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = (uint32_t)wave_incl_scan((int)v, lane);
    __syncthreads();                                                        // the previous use of sums is over
    if (lane == 63) sums[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kCodeWaves; ++w) {
        if (w < wave) base += sums[w];
        total += sums[w];
    }
    return base + incl - v;
}

// block l of image im's scan: its coefficients, the block whose DC predicts its own (nullptr: 0), its component
__device__ __forceinline__ void locate(const HuffImg& im, uint32_t l, const int16_t* __restrict__ coef, const int16_t*& blk, const int16_t*& prev,
                                       int& ci) {
    const uint32_t mcu = l / (uint32_t)im.bpm;
    const int r = (int)(l - mcu * (uint32_t)im.bpm), ny = im.h0 * im.v0;
    ci = r < ny ? 0 : r - ny + 1;
    const int h = ci ? 1 : im.h0, v = ci ? 1 : im.v0, q = ci ? 0 : r;
    const int16_t* const plane = coef + im.coef_base + im.coef_off[ci];
    const long long wb = im.wblocks[ci];
    auto at = [&](uint32_t m, int k) {
        const uint32_t my = m / (uint32_t)im.mcux, mx = m - my * (uint32_t)im.mcux;
        const int y = k / h, x = k - y * h;
        return plane + (((long long)my * v + y) * wb + (long long)mx * h + x) * 64;
    };
    blk = at(mcu, q);
    prev = q > 0 ? at(mcu, q - 1) : mcu > 0 ? at(mcu - 1, h * v - 1) : nullptr;
}

__device__ __forceinline__ int bit_length(unsigned v) { return v ? 32 - __clz(v) : 0; }

// encode_block's rule for the lane at zigzag position `lane` holding coefficient c: its code (right-aligned, MSB first) and its length.
// nz = the ballot of the non-zero lanes; pred = the DC predictor; bad is set for a size without a code (the table index is clamped first).
__device__ __forceinline__ int lane_code(const uint32_t* __restrict__ tab, int ci, int lane, int c, int pred, unsigned long long nz,
                                         unsigned long long& code, bool& bad) {
    code = 0;
    bad = false;
    if (lane == 0) {
        const int diff = c - pred, t = diff < 0 ? -diff : diff, t2 = diff < 0 ? diff - 1 : diff;
        int n = bit_length((unsigned)t);
        bad = n > 11;
        n = min(n, 11);
        const uint32_t e = tab[(ci ? 256 : 0) + n];
        code = ((unsigned long long)(e & 0xFFFFu) << n) | ((unsigned)t2 & ((1u << n) - 1));
        return (int)(e >> 16) + n;
    }
    const uint32_t* const ac = tab + (ci ? 768 : 512);
    if (c == 0) {
        if (lane != 63) return 0;
        const uint32_t e = ac[0];                                           // EOB: the last coefficient is zero
        code = e & 0xFFFFu;
        return (int)(e >> 16);
    }
    const unsigned long long below = nz & ((1ull << lane) - 1) & ~1ull;     // the non-zero AC positions in front of this one
    const int prev = below ? 63 - __clzll((long long)below) : 0;
    const int run = lane - prev - 1, t = c < 0 ? -c : c, t2 = c < 0 ? c - 1 : c;
    int n = bit_length((unsigned)t);
    bad = n > 10;
    n = min(n, 10);
    const uint32_t e = ac[((run & 15) << 4) | n], z = ac[0xF0];
    const int zl = (int)(z >> 16), zr = run >> 4;                           // zr <= 3
    int len = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < zr) { code = (code << zl) | (z & 0xFFFFu); len += zl; }
    const int el = (int)(e >> 16) + n;
    code = (code << el) | ((unsigned long long)(e & 0xFFFFu) << n) | ((unsigned)t2 & ((1u << n) - 1));
    return len + el;
}

// ------------------------------------------------------------------------------------------
// Size pass: one wave per block, kWaveBlocks consecutive blocks of the batch per wave (the search for the image is paid once; the walk
// to the next image is bounded by the table's entries), kCodeWaves waves per workgroup.  bits[g] = the block's bits; fail[i] |= 1 for an
// image with a coefficient that has no code.  No LDS, no barrier: a wave behind the last block leaves.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLanes) void huff_size_kernel(const HuffImg* __restrict__ imgs, const long long* __restrict__ start, int n,
                                                           const uint32_t* __restrict__ tab, const int16_t* __restrict__ coef, long long B,
                                                           uint32_t* __restrict__ bits, int* __restrict__ fail) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, zz = kZigzag[lane];
    const long long g0 = ((long long)blockIdx.x * kCodeWaves + wave) * kWaveBlocks;
    if (g0 >= B) return;
    int i = find_entry(start, n, g0);
    long long hi = start[i + 1];
    for (int k = 0; k < kWaveBlocks; ++k) {
        const long long g = g0 + k;
        if (g >= B) break;
        while (g >= hi) hi = start[++i + 1];                                // g < B = start[n]: ends at an entry below n
        const int16_t *blk, *prev;
        int ci;
        locate(imgs[i], (uint32_t)(g - start[i]), coef, blk, prev, ci);
        const int c = blk[zz], pred = prev ? prev[0] : 0;
        const unsigned long long nz = __ballot(c != 0);
        unsigned long long code;
        bool bad;
        const int len = lane_code(tab, ci, lane, c, pred, nz, code, bad);
        const int incl = wave_incl_scan(len, lane);
        if (lane == 63) bits[g] = (uint32_t)incl;
        if (__ballot(bad) != 0 && lane == 0) atomicOr(&fail[i], 1);
    }
}

// ------------------------------------------------------------------------------------------
// The scan: out[0 .. N] = exclusive prefix sum of in[0 .. N), 64-bit, in three launches.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLanes) void scan_reduce_kernel(const uint32_t* __restrict__ in, long long N, unsigned long long* __restrict__ partial) {
    __shared__ uint32_t sums[kCodeWaves];
    const long long at = ((long long)blockIdx.x * kLanes + threadIdx.x) * 4;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (at + k < N) v += in[at + k];
    uint32_t total;
    block_excl_scan(v, sums, total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// ONE workgroup: partial[0 .. P) -> its exclusive prefix sum in place, the grand total -> *total.  A lane walks its own run of
// ceil(P / kLanes) entries; lane 0 adds up the kLanes run sums.
__global__ __launch_bounds__(kLanes) void scan_partials_kernel(unsigned long long* __restrict__ partial, long long P, unsigned long long* __restrict__ total) {
    __shared__ unsigned long long runs[kLanes];
    const long long per = (P + kLanes - 1) / kLanes, lo = min(P, per * (long long)threadIdx.x), hi = min(P, lo + per);
    unsigned long long sum = 0;
    for (long long k = lo; k < hi; ++k) sum += partial[k];
    runs[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long acc = 0;
        for (int k = 0; k < kLanes; ++k) { const unsigned long long r = runs[k]; runs[k] = acc; acc += r; }
        *total = acc;
    }
    __syncthreads();
    unsigned long long acc = runs[threadIdx.x];
    for (long long k = lo; k < hi; ++k) { const unsigned long long r = partial[k]; partial[k] = acc; acc += r; }
}

__global__ __launch_bounds__(kLanes) void scan_apply_kernel(const uint32_t* __restrict__ in, long long N, const unsigned long long* __restrict__ partial,
                                                            unsigned long long* __restrict__ out) {
    __shared__ uint32_t sums[kCodeWaves];
    const long long at = ((long long)blockIdx.x * kLanes + threadIdx.x) * 4;
    uint32_t x[4], v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[k] = at + k < N ? in[at + k] : 0; v += x[k]; }
    uint32_t total;
    unsigned long long acc = partial[blockIdx.x] + block_excl_scan(v, sums, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (at + k < N) out[at + k] = acc;
        acc += x[k];
    }
}

// totals[i] = off[start[i + 1]] - off[start[i]]: what image i's entries add up to
__global__ __launch_bounds__(kLanes) void huff_totals_kernel(const unsigned long long* __restrict__ off, const long long* __restrict__ start, int n,
                                                             unsigned long long* __restrict__ totals) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i < n) totals[i] = off[start[i + 1]] - off[start[i]];
}

// What the stuffing passes know of an image: raw_off < 0 = no stream (a skipped or a failed image: no chunk points at it).
struct Place {
    long long raw_off, raw_bytes;                    // the unstuffed stream in the raw buffer (16-byte aligned), its size
};

// code's low `len` bits (1 <= len <= 59) into the stream held in `words` (word w = stream bits 32 w .. 32 w + 31, MSB first) at bit pos
__device__ __forceinline__ void or_bits(uint32_t* words, unsigned pos, unsigned long long code, int len) {
    const unsigned long long c = code << (64 - len);                       // left-aligned
    const unsigned wi = pos >> 5, b = pos & 31;
    const uint32_t a0 = (uint32_t)(c >> (32 + b)), a1 = (uint32_t)((c << (32 - b)) >> 32), a2 = b ? (uint32_t)((c << (64 - b)) >> 32) : 0;
    if (a0) atomicOr(&words[wi], a0);                                      // (a word without one-bits may lie behind the block's words)
    if (a1) atomicOr(&words[wi + 1], a1);
    if (a2) atomicOr(&words[wi + 2], a2);
}

// ------------------------------------------------------------------------------------------
// Pack pass: the size pass's mapping and codes; every wave of the workgroup passes the barriers of all kWaveBlocks turns, with nothing
// to do behind the last block or for an image without a stream.  raw is zero where no code lands.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLanes) void huff_pack_kernel(const HuffImg* __restrict__ imgs, const long long* __restrict__ start, int n,
                                                           const uint32_t* __restrict__ tab, const int16_t* __restrict__ coef, long long B,
                                                           const unsigned long long* __restrict__ off, const Place* __restrict__ place,
                                                           uint32_t* __restrict__ raw) {
    __shared__ uint32_t words[kCodeWaves][kBlockWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, zz = kZigzag[lane];
    const long long g0 = ((long long)blockIdx.x * kCodeWaves + wave) * kWaveBlocks;
    int i = g0 < B ? find_entry(start, n, g0) : 0;
    long long hi = g0 < B ? start[i + 1] : 0;
    for (int k = 0; k < kWaveBlocks; ++k) {                                 // the same count for every wave: two barriers per turn
        const long long g = g0 + k;
        unsigned long long code = 0;
        int len = 0, excl = 0, total = 0, pad = 0, nw = 0;
        unsigned shift = 0;
        long long w0 = 0;
        if (g < B) {
            while (g >= hi) hi = start[++i + 1];                            // as the size pass
            if (place[i].raw_off >= 0) {
                const int16_t *blk, *prev;
                int ci;
                locate(imgs[i], (uint32_t)(g - start[i]), coef, blk, prev, ci);
                const int c = blk[zz], pred = prev ? prev[0] : 0;
                const unsigned long long nz = __ballot(c != 0);
                bool bad;
                len = lane_code(tab, ci, lane, c, pred, nz, code, bad);
                const int incl = wave_incl_scan(len, lane);
                excl = incl - len;
                total = __shfl(incl, 63);
                const unsigned long long at = off[g] - off[start[i]];       // the block's first bit in its image's stream
                if (g + 1 == hi) pad = (int)((8 - ((at + (unsigned)total) & 7)) & 7);
                shift = (unsigned)(at & 31);
                w0 = place[i].raw_off / 4 + (long long)(at >> 5);
                nw = (int)((shift + (unsigned)total + (unsigned)pad + 31) >> 5);   // <= 54
            }
        }
        if (lane < nw) words[wave][lane] = 0;
        __syncthreads();
        if (len > 0) or_bits(words[wave], shift + (unsigned)excl, code, len);
        if (pad > 0 && lane == 0) or_bits(words[wave], shift + (unsigned)total, (1ull << pad) - 1, pad);
        __syncthreads();
        if (lane < nw) {
            const uint32_t w = __builtin_bswap32(words[wave][lane]);        // stream byte order
            if (lane == 0 || lane == nw - 1) atomicOr(&raw[w0 + lane], w);
            else raw[w0 + lane] = w;
        }
        __syncthreads();                                                    // the words are read before the next turn zeroes them
    }
}

// the lane's dword of chunk q of a stream and how many of its bytes belong to the stream (0..4)
__device__ __forceinline__ uint32_t stream_word(const uint8_t* __restrict__ raw, const Place& p, long long q, long long& j, int& valid) {
    j = q * kStuffChunk + (long long)threadIdx.x * 4;
    valid = (int)max(0LL, min(4LL, p.raw_bytes - j));
    return valid ? *reinterpret_cast<const uint32_t*>(raw + p.raw_off + j) : 0u;
}

// ff[c] = the 0xFF bytes of chunk c (chunk_start maps the workgroup to its image)
__global__ __launch_bounds__(kLanes) void huff_ff_kernel(const Place* __restrict__ place, const long long* __restrict__ chunk_start, int n,
                                                         const uint8_t* __restrict__ raw, uint32_t* __restrict__ ff) {
    __shared__ uint32_t sums[kCodeWaves];
    const long long c = blockIdx.x;
    const int i = find_entry(chunk_start, n, c);
    long long j;
    int valid;
    const uint32_t w = stream_word(raw, place[i], c - chunk_start[i], j, valid);
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt += k < valid && ((w >> (8 * k)) & 255u) == 255u;
    uint32_t total;
    block_excl_scan(cnt, sums, total);
    if (threadIdx.x == 0) ff[c] = total;
}

// What the assembling pass knows of an image besides its Place; the header bytes follow the rows, kHdrSlot per image.
struct FileAt {
    long long off, size;                             // of the file in the arena
    int32_t hdr_len, pad_;
};

// ------------------------------------------------------------------------------------------
// Assemble: stream byte j of a file lands at header + j + the 0xFF bytes in front of it (those of the chunks in front: ffoff; those of
// this chunk: a workgroup prefix sum), followed by a zero when it is 0xFF.  Byte stores: the positions are unaligned by nature.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLanes) void huff_file_kernel(const Place* __restrict__ place, const long long* __restrict__ chunk_start, int n,
                                                           const uint8_t* __restrict__ raw, const unsigned long long* __restrict__ ffoff,
                                                           const FileAt* __restrict__ files, const uint8_t* __restrict__ hdrs,
                                                           uint8_t* __restrict__ arena) {
    __shared__ uint32_t sums[kCodeWaves];
    const long long c = blockIdx.x;
    const int i = find_entry(chunk_start, n, c);
    const FileAt f = files[i];
    long long j;
    int valid;
    const uint32_t w = stream_word(raw, place[i], c - chunk_start[i], j, valid);
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt += k < valid && ((w >> (8 * k)) & 255u) == 255u;
    uint32_t total;
    const uint32_t excl = block_excl_scan(cnt, sums, total);
    uint8_t* const file = arena + f.off;
    uint8_t* out = file + f.hdr_len + j + (long long)(ffoff[c] - ffoff[chunk_start[i]]) + excl;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= valid) break;
        const uint32_t b = (w >> (8 * k)) & 255u;
        *out++ = (uint8_t)b;
        if (b == 255u) *out++ = 0;
    }
    if (c == chunk_start[i])
        for (int k = threadIdx.x; k < f.hdr_len; k += kLanes) file[k] = hdrs[(size_t)i * kHdrSlot + k];
    if (c + 1 == chunk_start[i + 1] && threadIdx.x == 0) { file[f.size - 2] = 0xFF; file[f.size - 1] = 0xD9; }
}

// out[0 .. N] = exclusive prefix sum of in[0 .. N) on s; partial holds ceil(N / kScanChunk) entries
void scan(const uint32_t* in, long long N, unsigned long long* partial, unsigned long long* out, hipStream_t s) {
    const long long P = (N + kScanChunk - 1) / kScanChunk;
    hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)P), dim3(kLanes), 0, s, in, N, partial);
    hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kLanes), 0, s, partial, P, out + N);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)P), dim3(kLanes), 0, s, in, N, static_cast<const unsigned long long*>(partial), out);
}

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

JpegHuff::~JpegHuff() {
    if (h_totals_) (void)hipHostFree(h_totals_);
}

int JpegHuff::code(const fh_jpeg_desc* descs, int n, const int16_t* d_coef, const long long* coef_base, fh_blob* files, int* status, hipStream_t s) {
    // ---- the size pass and its scan
    const size_t geom_bytes = (size_t)n * sizeof(HuffImg) + ((size_t)n + 1) * sizeof(long long) + 1024 * sizeof(uint32_t);
    uint8_t* h = static_cast<uint8_t*>(geom_.stage(geom_bytes));
    HuffImg* const rows = reinterpret_cast<HuffImg*>(h);
    long long* const start = reinterpret_cast<long long*>(h + (size_t)n * sizeof(HuffImg));
    jpeg_huff_codes(reinterpret_cast<uint32_t*>(start + n + 1));
    long long B = 0;
    for (int i = 0; i < n; ++i) {
        files[i] = fh_blob{nullptr, 0};
        const bool live = coef_base[i] >= 0;
        if (status) status[i] = live ? 0 : 1;
        HuffImg& r = rows[i];
        memset(&r, 0, sizeof(r));
        start[i] = B;
        if (!live) continue;
        const fh_jpeg_desc& d = descs[i];
        r.coef_base = coef_base[i];
        r.ncomp = d.ncomp; r.h0 = d.comp[0].h; r.v0 = d.comp[0].v;
        r.mcux = d.comp[0].wblocks / d.comp[0].h;
        r.bpm = r.h0 * r.v0 + (d.ncomp - 1);
        for (int ci = 0; ci < d.ncomp; ++ci) {
            r.coef_off[ci] = d.comp[ci].coef_off; r.wblocks[ci] = d.comp[ci].wblocks;
            B += (long long)d.comp[ci].wblocks * d.comp[ci].hblocks;
        }
    }
    start[n] = B;
    used_ = 0;
    blocks_ = 0;
    if (B == 0) return 0;                                                  // every slot skipped
    if (B > 0x7FFFFFFFLL) throw std::runtime_error("fh_jpeg_code_batch_dev: the batch has 2^31 blocks or more");
    const long long P = (B + kScanChunk - 1) / kScanChunk;
    bits_.ensure((size_t)B * sizeof(uint32_t));
    off_.ensure(((size_t)B + 1) * sizeof(unsigned long long));
    partial_.ensure((size_t)P * sizeof(unsigned long long));
    const size_t totals_bytes = (size_t)n * (sizeof(unsigned long long) + sizeof(int));
    totals_.ensure(totals_bytes);
    if (h_totals_bytes_ < totals_bytes) {
        if (h_totals_) (void)hipHostFree(h_totals_);
        h_totals_ = nullptr; h_totals_bytes_ = 0;
        FH_HIP(hipHostMalloc(&h_totals_, totals_bytes, hipHostMallocDefault));
        h_totals_bytes_ = totals_bytes;
    }
    unsigned long long* const d_totals = totals_.as<unsigned long long>();
    int* const d_fail = reinterpret_cast<int*>(d_totals + n);
    const uint8_t* dev = static_cast<const uint8_t*>(geom_.send(geom_bytes, s));
    const HuffImg* const d_rows = reinterpret_cast<const HuffImg*>(dev);
    const long long* const d_start = reinterpret_cast<const long long*>(dev + (size_t)n * sizeof(HuffImg));
    const uint32_t* const d_tab = reinterpret_cast<const uint32_t*>(d_start + n + 1);
    const unsigned code_groups = (unsigned)((B + kCodeWaves * kWaveBlocks - 1) / (kCodeWaves * kWaveBlocks)), img_groups = (unsigned)((n + kLanes - 1) / kLanes);
    FH_HIP(hipMemsetAsync(d_fail, 0, (size_t)n * sizeof(int), s));
    hipLaunchKernelGGL(huff_size_kernel, dim3(code_groups), dim3(kLanes), 0, s, d_rows, d_start, n, d_tab, d_coef, B, bits_.as<uint32_t>(), d_fail);
    scan(bits_.as<const uint32_t>(), B, partial_.as<unsigned long long>(), off_.as<unsigned long long>(), s);
    hipLaunchKernelGGL(huff_totals_kernel, dim3(img_groups), dim3(kLanes), 0, s, off_.as<const unsigned long long>(), d_start, n, d_totals);
    FH_HIP(hipGetLastError());
    FH_HIP(hipMemcpyAsync(h_totals_, d_totals, totals_bytes, hipMemcpyDeviceToHost, s));
    FH_HIP(hipStreamSynchronize(s));                                       // the first of two
    blocks_ = B;

    // ---- the streams: placed, zeroed, packed, their 0xFF bytes counted
    const size_t place_bytes = (size_t)n * sizeof(Place) + ((size_t)n + 1) * sizeof(long long);
    h = static_cast<uint8_t*>(place_.stage(place_bytes));
    Place* const place = reinterpret_cast<Place*>(h);
    long long* const chunk_start = reinterpret_cast<long long*>(h + (size_t)n * sizeof(Place));
    size_t raw_bytes = 0;
    long long chunks = 0;
    int coded = 0;
    {
        const unsigned long long* const img_bits = static_cast<const unsigned long long*>(h_totals_);
        const int* const fail = reinterpret_cast<const int*>(img_bits + n);
        for (int i = 0; i < n; ++i) {
            place[i] = Place{-1, 0};
            chunk_start[i] = chunks;
            if (coef_base[i] < 0) continue;
            if (fail[i]) { if (status) status[i] = FH_ERR_ARG; continue; }
            place[i] = Place{(long long)raw_bytes, (long long)((img_bits[i] + 7) / 8)};
            raw_bytes += align16((size_t)place[i].raw_bytes);
            chunks += (place[i].raw_bytes + kStuffChunk - 1) / kStuffChunk;
            ++coded;
        }
        chunk_start[n] = chunks;
    }
    if (coded == 0) return 0;
    if (chunks > 0x7FFFFFFFLL) throw std::runtime_error("fh_jpeg_code_batch_dev: the streams are too large for one launch");
    const long long Pc = (chunks + kScanChunk - 1) / kScanChunk;
    raw_.ensure(raw_bytes);
    ff_.ensure((size_t)chunks * sizeof(uint32_t));
    ffoff_.ensure(((size_t)chunks + 1) * sizeof(unsigned long long));
    partial_.ensure((size_t)Pc * sizeof(unsigned long long));
    dev = static_cast<const uint8_t*>(place_.send(place_bytes, s));
    const Place* const d_place = reinterpret_cast<const Place*>(dev);
    const long long* const d_chunk = reinterpret_cast<const long long*>(dev + (size_t)n * sizeof(Place));
    FH_HIP(hipMemsetAsync(raw_.p, 0, raw_bytes, s));
    hipLaunchKernelGGL(huff_pack_kernel, dim3(code_groups), dim3(kLanes), 0, s, d_rows, d_start, n, d_tab, d_coef, B,
                       off_.as<const unsigned long long>(), d_place, raw_.as<uint32_t>());
    hipLaunchKernelGGL(huff_ff_kernel, dim3((unsigned)chunks), dim3(kLanes), 0, s, d_place, d_chunk, n, raw_.as<const uint8_t>(), ff_.as<uint32_t>());
    scan(ff_.as<const uint32_t>(), chunks, partial_.as<unsigned long long>(), ffoff_.as<unsigned long long>(), s);
    hipLaunchKernelGGL(huff_totals_kernel, dim3(img_groups), dim3(kLanes), 0, s, ffoff_.as<const unsigned long long>(), d_chunk, n, d_totals);
    FH_HIP(hipGetLastError());
    FH_HIP(hipMemcpyAsync(h_totals_, d_totals, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    FH_HIP(hipStreamSynchronize(s));                                       // the second

    // ---- the files: sized, laid back to back, assembled
    const size_t files_bytes = (size_t)n * sizeof(FileAt) + (size_t)n * kHdrSlot;
    h = static_cast<uint8_t*>(files_.stage(files_bytes));
    FileAt* const at = reinterpret_cast<FileAt*>(h);
    uint8_t* const hdrs = h + (size_t)n * sizeof(FileAt);
    const unsigned long long* const img_ff = static_cast<const unsigned long long*>(h_totals_);
    size_t arena_bytes = 0;
    for (int i = 0; i < n; ++i) {
        at[i] = FileAt{0, 0, 0, 0};
        if (place[i].raw_off < 0) continue;
        size_t hdr = 0;
        if (fh_jpeg_write_header(&descs[i], hdrs + (size_t)i * kHdrSlot, kHdrSlot, &hdr) != 0)
            throw std::runtime_error("fh_jpeg_code_batch_dev: the header does not fit its slot");
        at[i] = FileAt{(long long)arena_bytes, (long long)(hdr + (size_t)place[i].raw_bytes + (size_t)img_ff[i] + 2), (int32_t)hdr, 0};
        arena_bytes += (size_t)at[i].size;
    }
    arena_.ensure(arena_bytes);
    used_ = arena_bytes;
    for (int i = 0; i < n; ++i)
        if (place[i].raw_off >= 0) files[i] = fh_blob{arena_.as<unsigned char>() + at[i].off, (size_t)at[i].size};
    dev = static_cast<const uint8_t*>(files_.send(files_bytes, s));
    hipLaunchKernelGGL(huff_file_kernel, dim3((unsigned)chunks), dim3(kLanes), 0, s, d_place, d_chunk, n, raw_.as<const uint8_t>(),
                       ffoff_.as<const unsigned long long>(), reinterpret_cast<const FileAt*>(dev), dev + (size_t)n * sizeof(FileAt),
                       arena_.as<uint8_t>());
    FH_HIP(hipGetLastError());
    return coded;
}

}  // namespace fh
