// face_iou.h — FaceDetector::iou (src/face_detector.cpp:340-354), the ONE device definition: integer intersection, integer denominator,
// one float divide.  Boxes are (x, y, width, height) in an int4.  0 / 0 is NaN, which fails every strict `iou > thr`.  Shared by the NMS
// (face_kernels.hip) and the tracker (track.hip); both files are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace fh {

__device__ __forceinline__ float iou_int(int4 a, int4 b) {
    const int x1 = max(a.x, b.x), y1 = max(a.y, b.y);
    const int x2 = min(a.x + a.z, b.x + b.z), y2 = min(a.y + a.w, b.y + b.w);
    const int w = max(0, x2 - x1), h = max(0, y2 - y1);
    const int inter = w * h;
    const int area1 = a.z * a.w, area2 = b.z * b.w;
    return (float)inter / (float)(area1 + area2 - inter);
}

}  // namespace fh
