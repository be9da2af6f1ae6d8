"""Template pooling (fh_gallery_fuse_ids) measured on one labelled gallery: --rows x 512, --templates clustered templates per identity
(centre + noise, shuffled), one process.
  (a) fuse_ids end to end (a synchronous call: host clock around it), and fh_gallery_group_ids alone on the same ids (host clock); the
      sum kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of `--profile N` (pass the kernel's average in
      us with --sum-kernel-us / --self-kernel-us and the table prints its bytes/s);
  (b) identity top-k through topk_ids_dev on the template gallery against row top-k on the fused gallery in fp32 and in F16_RERANK,
      alternated round by round, HIP events around blocks of 10 calls; and the share of queries whose identity list is the same;
  (c) self_scores_dev of the template gallery against the fused one.
One JSON line per point; --md FILE writes the tables."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--templates", type=int, default=8)
ap.add_argument("--q", type=int, nargs="+", default=[64, 256])
ap.add_argument("--k", type=int, default=16)
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--fuses", type=int, default=7)
ap.add_argument("--profile", type=int, default=0)
ap.add_argument("--sum-kernel-us", type=float, default=0.0)
ap.add_argument("--self-kernel-us", type=float, default=0.0)
ap.add_argument("--md", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402

DIM = 512


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def block_times(call, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range((calls + 9) // 10):
        e0.record()
        for _ in range(10):
            call()
        e1.record(); e1.synchronize()
        per.append(e0.elapsed_time(e1) / 10)
    return per


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "samples": len(v)}


def wall_ms(call, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t))
    return out


def fmt(s):
    return f"{s['median_ms']:.3f} ({s['min_ms']:.3f}-{s['max_ms']:.3f})"


def main():
    torch.cuda.set_device(0)
    G, T, k = a.rows, a.templates, a.k
    gen = torch.Generator(device="cuda").manual_seed(11)
    m = G // T
    centres = unit(torch.randn((m, DIM), device="cuda", generator=gen))
    rows = unit(centres.repeat_interleave(T, 0) + 0.02 * torch.randn((m * T, DIM), device="cuda", generator=gen))
    ids = (torch.arange(m, device="cuda") * 5 + 2).repeat_interleave(T).to(torch.int32)
    o = torch.randperm(m * T, device="cuda", generator=gen)
    rows, ids = rows[o].contiguous(), ids[o].contiguous()
    G = m * T
    src = fa.Gallery(DIM)
    src.upload(rows.data_ptr(), G, True, 0, ids_ptr=ids.data_ptr())
    f32, f16 = fa.Gallery(DIM), fa.Gallery(DIM, scan="f16")
    ids_host = ids.cpu().numpy()
    scores = torch.zeros(G, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    if a.profile:                                              # for a kernel-trace run: nothing but the calls
        for _ in range(a.profile):
            src.fuse(f32)
            src.self_scores_dev(f32, scores.data_ptr(), st)
        torch.cuda.synchronize()
        return

    out = []
    # (a) fuse_ids and its host grouping
    src.fuse(f32); src.fuse(f16)                               # warm-up: buffers sized, code loaded
    assert len(f32) == m and len(f16) == m
    d = {"what": "fuse_ids", "rows": G, "dim": DIM, "templates": T, "identities": m,
         "fuse_fp32_dst": stats(wall_ms(lambda: src.fuse(f32), a.fuses)), "fuse_f16_dst": stats(wall_ms(lambda: src.fuse(f16), a.fuses)),
         "group_ids_host": stats(wall_ms(lambda: fa.group_ids(ids_host), a.fuses)),
         "sum_kernel_bytes": G * DIM * 4 + m * DIM * 4 + G * 4 + m * 16}
    if a.sum_kernel_us:
        d["sum_kernel_us"] = a.sum_kernel_us
        d["sum_kernel_TBps"] = round(d["sum_kernel_bytes"] / (a.sum_kernel_us * 1e-6) / 1e12, 3)
    print(json.dumps(d), flush=True)
    out.append(d)

    # (b) identity top-k on the templates against row top-k on the pooled rows
    for Q in a.q:
        pick = torch.randint(0, m, (Q,), device="cuda", generator=gen)
        q = unit(centres[pick] + 0.02 * torch.randn((Q, DIM), device="cuda", generator=gen)).contiguous()
        sc = torch.zeros((Q, k), device="cuda"); ix = torch.zeros((Q, k), dtype=torch.int32, device="cuda"); rw = torch.zeros_like(ix)
        sides = {"topk_ids_on_templates": lambda: src.topk_ids_dev(q.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), rw.data_ptr(), st),
                 "topk_on_fused_fp32": lambda: f32.topk_dev(q.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), st),
                 "topk_on_fused_f16": lambda: f16.topk_dev(q.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), st)}
        res = {name: [] for name in sides}
        for call in sides.values():
            block_times(call, 20)
        f16.scan_stats()
        for _ in range(a.rounds):                              # alternated
            for name, call in sides.items():
                res[name] += block_times(call, (a.calls + a.rounds - 1) // a.rounds)
        cert, fb = f16.scan_stats()
        # the same people?  identity lists of the template gallery against the ids of the fused gallery's rows
        sides["topk_ids_on_templates"](); torch.cuda.synchronize()
        want = ix.cpu().numpy().copy()
        f32.topk_ids_dev(q.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), rw.data_ptr(), st); torch.cuda.synchronize()
        got = ix.cpu().numpy().copy()
        d = {"what": "topk", "rows": G, "fused_rows": m, "Q": Q, "k": k, **{name: stats(v) for name, v in res.items()},
             "f16_certified_share": round(cert / max(cert + fb, 1), 4),
             "same_top1": round(float((want[:, 0] == got[:, 0]).mean()), 4),
             "same_list_in_order": round(float((want == got).all(1).mean()), 4),
             "same_set": round(float(np.mean([set(w) == set(g) for w, g in zip(want, got)])), 4),
             "mean_overlap": round(float(np.mean([len(set(w) & set(g)) / k for w, g in zip(want, got)])), 4)}
        print(json.dumps(d), flush=True)
        out.append(d)

    # (c) the mislabel audit
    block_times(lambda: src.self_scores_dev(f32, scores.data_ptr(), st), 20)
    d = {"what": "self_scores", "rows": G, "fused_rows": m,
         "self_scores": stats(block_times(lambda: src.self_scores_dev(f32, scores.data_ptr(), st), a.calls)),
         "bytes": G * DIM * 4 + m * DIM * 4 + G * 8}          # every row of both galleries once, ids in, scores out
    d["TBps_of_call"] = round(d["bytes"] / (d["self_scores"]["median_ms"] * 1e-3) / 1e12, 3)
    if a.self_kernel_us:
        d["self_kernel_us"] = a.self_kernel_us
    print(json.dumps(d), flush=True)
    out.append(d)

    if a.md:
        with open(a.md, "w") as fo:
            f = out[0]
            fo.write(f"fuse_ids, {f['rows']} x {f['dim']}, {f['templates']} templates per identity -> {f['identities']} rows "
                     f"(median (min-max) ms over {a.fuses} calls, host clock around the synchronous call):\n\n")
            fo.write("| part | ms |\n|---|---|\n")
            fo.write(f"| fuse_ids, fp32 dst | {fmt(f['fuse_fp32_dst'])} |\n| fuse_ids, F16_RERANK dst | {fmt(f['fuse_f16_dst'])} |\n")
            fo.write(f"| fh_gallery_group_ids alone (host) | {fmt(f['group_ids_host'])} |\n")
            if a.sum_kernel_us:
                fo.write(f"| fuse_sum_kernel (kernel trace) | {a.sum_kernel_us / 1e3:.3f}: {f['sum_kernel_bytes'] / 1e9:.3f} GB -> {f['sum_kernel_TBps']:.2f} TB/s |\n")
            fo.write("\n| Q | k | topk_ids on templates ms | topk on fused fp32 ms | topk on fused F16_RERANK ms | certified | same top-1 | same list | same set | mean overlap |\n")
            fo.write("|---|---|---|---|---|---|---|---|---|---|\n")
            for d in out[1:-1]:
                fo.write(f"| {d['Q']} | {d['k']} | {fmt(d['topk_ids_on_templates'])} | {fmt(d['topk_on_fused_fp32'])} | {fmt(d['topk_on_fused_f16'])} | "
                         f"{100 * d['f16_certified_share']:.1f}% | {100 * d['same_top1']:.1f}% | {100 * d['same_list_in_order']:.1f}% | "
                         f"{100 * d['same_set']:.1f}% | {100 * d['mean_overlap']:.1f}% |\n")
            s = out[-1]
            fo.write(f"\nself_scores_dev, {s['rows']} rows against {s['fused_rows']}: {fmt(s['self_scores'])} ms per call, "
                     f"{s['bytes'] / 1e9:.3f} GB -> {s['TBps_of_call']:.2f} TB/s of the call\n")


if __name__ == "__main__":
    main()
