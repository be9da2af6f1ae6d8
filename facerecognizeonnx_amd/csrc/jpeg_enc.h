// jpeg_enc.h — the forward path of the JPEG encoder on the device (jpeg_enc.hip): the object behind fh_jpegenc's launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/facehip.h"
#include "engine.h"

namespace fh {

// Owns the device image of a call's descriptor table (StagedTable: one asynchronous copy per call, a ring of pinned staging buffers) and
// the workspace the sample kernel writes the components' u8 planes to.  Both grow on demand.
class JpegEnc {
  public:
    // fh_jpeg_forward_batch_dev's body, arguments already checked (every live frame's descriptor through fh_jpeg_enc_check, its rows /
    // cols / step against the descriptor): two launches on s, whatever n is.
    void forward(const fh_jpeg_desc* descs, int n, const FrameIn* frames, int16_t* d_coef, const long long* coef_base, hipStream_t s);

  private:
    StagedTable table_;
    DevBuf planes_;
};

// image_io.cpp: the host writer's code tables, [DC0, DC1, AC0, AC1][256] entries of length << 16 | code
void jpeg_huff_codes(uint32_t* tab);

// The Huffman coder on the device (jpeg_huff.hip): owns the staged tables of a call, the per-block bit counts and offsets, the unstuffed
// streams, the 0xFF counts and the byte arena the files are assembled in.  All grow on demand.
class JpegHuff {
  public:
    JpegHuff() = default;
    JpegHuff(const JpegHuff&) = delete;
    JpegHuff& operator=(const JpegHuff&) = delete;
    ~JpegHuff();
    // fh_jpeg_code_batch_dev's body, arguments already checked (every live descriptor through fh_jpeg_enc_check; live = coef_base[i] >= 0):
    // files[i] = {device pointer into the arena, size} and status[i] (0 coded, 1 skipped, FH_ERR_ARG uncodable) for every slot; returns the
    // number of files coded.  Synchronises s twice; the assembling kernel is asynchronous on s.
    int code(const fh_jpeg_desc* descs, int n, const int16_t* d_coef, const long long* coef_base, fh_blob* files, int* status, hipStream_t s);
    const DevBuf& arena() const { return arena_; }
    size_t arena_used() const { return used_; }                            // bytes of the last call's files
    const DevBuf& bits() const { return bits_; }
    long long blocks() const { return blocks_; }                           // of the last call: entries of bits()

  private:
    StagedTable geom_, place_, files_;                                     // the tables of the size / pack, the stuffing and the assembling passes
    DevBuf bits_, off_, partial_, totals_, raw_, ff_, ffoff_, arena_;
    void* h_totals_ = nullptr;                                             // pinned: what the two synchronisations bring back, a few bytes per image
    size_t h_totals_bytes_ = 0;
    size_t used_ = 0;
    long long blocks_ = 0;
};

}  // namespace fh
