// jpeg_dev.h — device reconstruction of JPEG coefficients (jpeg_dev.hip): the object behind fh_jpegdec's launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/facehip.h"
#include "engine.h"

namespace fh {

// Owns the device image of a call's descriptor table (StagedTable: one asynchronous copy per call, a ring of pinned staging buffers) and
// the workspace the IDCT kernel writes the components' u8 planes to.  Both grow on demand.
class JpegDev {
  public:
    // fh_jpeg_reconstruct_batch_dev's body, arguments already checked (every descriptor through fh_jpeg_desc_check, every live frame's
    // rows / cols / step against its descriptor): two launches on s, whatever n is.
    void reconstruct(const fh_jpeg_desc* descs, int n, const int16_t* d_coef, const long long* coef_base, const FrameIn* frames, hipStream_t s);

  private:
    StagedTable table_;
    DevBuf planes_;
};

}  // namespace fh
