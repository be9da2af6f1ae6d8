"""A numpy model of tiled detection (include/facehip.h, "tiled detection of large frames"): the tile plan and the per-frame merge, built
from the oracle's own row loop and NMS.  Independent of the library: the CPU tests hold fh_tile_plan to plan(), the GPU tests hold
the device's records to merge()."""
import numpy as np

from oracle import oracle

FACE_DTYPE = oracle.FACE_DTYPE


def axis(length, tile, overlap):
    """Origins and size of the tiles along one axis: integers only, the last tile shifted inward."""
    if length <= tile:
        return [0], length
    s = tile - overlap
    n = -(-(length - tile) // s) + 1
    return [min(j * s, length - tile) for j in range(n)], tile


def plan(rows, cols, tile_w, tile_h, overlap):
    """[(x, y, w, h, edges)]: view 0 the whole frame, then the tiles row-major (only when there is more than one); edges bit 0 left,
    1 top, 2 right, 3 bottom = interior.  An empty image has no views."""
    if rows <= 0 or cols <= 0:
        return []
    xs, w = axis(cols, tile_w, overlap)
    ys, h = axis(rows, tile_h, overlap)
    views = [(0, 0, cols, rows, 0)]
    if len(xs) * len(ys) == 1:
        return views
    for y in ys:
        for x in xs:
            views.append((x, y, w, h, (x > 0) | (y > 0) << 1 | (x + w < cols) << 2 | (y + h < rows) << 3))
    return views


def letterbox_scale(h, w, in_w, in_h):
    """FaceDetector::preprocess' float arithmetic (face_detector.cpp:101-113); 0.0 for a dead plan."""
    f = np.float32
    scale = min(f(in_w) / f(w), f(in_h) / f(h))
    nw, nh = int(f(w) * scale), int(f(h) * scale)
    return float(scale) if nw > 0 and nh > 0 else 0.0


def border_keep(c, view, border):
    """The border rule on candidates in VIEW coordinates: False where the box lies within `border` of an interior edge."""
    _, _, w, h, edges = view
    keep = np.ones(len(c), bool)
    if border < 0 or edges == 0:
        return keep
    x, y, bw, bh = (c[k].astype(np.int64) for k in ("x", "y", "w", "h"))
    if edges & 1:
        keep &= ~(x <= border)
    if edges & 2:
        keep &= ~(y <= border)
    if edges & 4:
        keep &= ~(x + bw >= w - border)
    if edges & 8:
        keep &= ~(y + bh >= h - border)
    return keep


def candidates(view_rows, views, in_w, in_h, border, score_thr):
    """Per view: (all thresholded candidates in view coordinates, the keep mask of the border rule, the kept ones shifted)."""
    out = []
    for v, (rows, view) in enumerate(zip(view_rows, views)):
        scale = letterbox_scale(view[3], view[2], in_w, in_h)
        c = oracle.threshold_rows(rows, scale, score_thr) if scale > 0 else np.zeros(0, FACE_DTYPE)
        keep = border_keep(c, view, border) if v > 0 else np.ones(len(c), bool)
        s = c[keep].copy()
        if v > 0:                                              # view 0 is at the origin and is left as it is
            s["x"] += np.int32(view[0]); s["y"] += np.int32(view[1])
            s["lm"][:, 0::2] += np.float32(view[0]); s["lm"][:, 1::2] += np.float32(view[1])
        out.append((c, keep, s))
    return out


def merge(view_rows, views, in_w, in_h, border, score_thr, nms_thr):
    """The records of one frame: view_rows[v] = the [N, >= 15] rows of view v (plan order).  oracle.nms orders by (score desc,
    position asc), which on the concatenation in plan order is (score desc, view asc, row asc)."""
    cs = candidates(view_rows, views, in_w, in_h, border, score_thr)
    allc = np.concatenate([s for _, _, s in cs]) if cs else np.zeros(0, FACE_DTYPE)
    return oracle.nms(allc, nms_thr) if len(allc) else allc
