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

}  // namespace fh
