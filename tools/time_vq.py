"""Times k-means vector quantisation (not a test): P rows of D = 45 columns against K = 4096 codes, on the SH rows of the C3
synthetic model and on uniform noise.

In ONE process after a warm-up, event-timed medians of
  assign      vq_assign (msgs_vq_assign: the layout kernel and the MFMA search), with its FLOP rate 2 P K D / time beside the f32
              matrix peak
  update      vq_update (sort, counts and offsets in torch, then msgs_vq_update), and msgs_vq_update alone on a prepared order
  torch       the same definition composed from torch ops: a chunked x @ c.T + argmin (chunks of `--torch-rows` rows, so that the
              [rows, K] score matrix fits) and index_add_ for the update
  kmeans      one 10-iteration compress.kmeans, and one save_compressed of the whole model with the file size beside the PLY's
    python tools/time_vq.py [--steps 10] [--warmup 3] [--rows 1000000] [--codes 4096] [--json out.json]
For the kernels' own times trace by themselves:
    rocprofv3 --kernel-trace --stats -- python tools/time_vq.py --steps 3 --only kernels"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import compress  # noqa: E402
import diff_gaussian_rasterization as dgr  # noqa: E402
import model_io  # noqa: E402
import scenes  # noqa: E402
from synthetic_model import SyntheticGaussians  # noqa: E402

F32_MATRIX_PEAK = 155e12           # FLOP/s: v_mfma_f32_32x32x2_f32 as measured on an MI355X (157.3 by specification)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def median_ms(fn, warmup, steps):
    ts = [timed(fn)[0] for _ in range(warmup + steps)][warmup:]
    return {"ms": round(float(np.median(ts)), 4), "p10_p90": [round(float(np.percentile(ts, q)), 4) for q in (10, 90)]}


def torch_assign(x, c, rows):
    n = 0.5 * (c * c).sum(1)
    out = torch.empty(len(x), dtype=torch.int64, device=x.device)
    for a in range(0, len(x), rows):
        out[a:a + rows] = torch.argmin(n[None, :] - x[a:a + rows] @ c.T, dim=1)
    return out


def torch_update(x, idx, c):
    num = torch.zeros_like(c).index_add_(0, idx, x)
    cnt = torch.zeros(len(c), device=x.device).index_add_(0, idx, torch.ones(len(x), device=x.device))
    return torch.where(cnt[:, None] > 0, num / cnt[:, None].clamp(min=1), c)


def raw_update(x, idx, c):
    """msgs_vq_update alone: the order, offsets and buffers are made once, outside the timed call"""
    P, D = x.shape
    K = len(c)
    order = torch.sort(idx, stable=True).indices
    members = torch.bincount(idx, minlength=K)
    zero = torch.zeros(1, dtype=torch.int64, device=x.device)
    offsets = torch.cat((zero, torch.cumsum(members, 0))).to(torch.int32)
    chunks = (members + (dgr.VQ_UPDATE_CHUNK - 1)) // dgr.VQ_UPDATE_CHUNK
    chunk_offsets = torch.cat((zero, torch.cumsum(chunks, 0))).to(torch.int32)
    new, mass = torch.empty_like(c), torch.empty(K, dtype=torch.float64, device=x.device)
    count = torch.empty(K, dtype=torch.int32, device=x.device)
    scratch = torch.empty(dgr._C.lib.msgs_vq_scratch_bytes(P, D, K), dtype=torch.uint8, device=x.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = (order, offsets, chunk_offsets, new, mass, count, scratch)
    return keep, lambda: dgr._C.check(dgr._C.lib.msgs_vq_update(
        P, D, K, ptr(x), None, ptr(order), ptr(offsets), ptr(chunk_offsets), ptr(c), ptr(new), ptr(mass), ptr(count), ptr(scratch),
        scratch.numel(), stream), "msgs_vq_update")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--codes", type=int, default=4096)
    ap.add_argument("--torch-rows", type=int, default=65536)
    ap.add_argument("--only", choices=("all", "kernels"), default="all")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sc, _, _ = scenes.config("C3")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    P, K = min(a.rows, pc._xyz.shape[0]), a.codes
    g = torch.Generator().manual_seed(0)
    data = {"c3_sh_rows": compress.sh_rows(pc)[:P].contiguous(), "uniform_noise": torch.rand(P, 45, generator=g).cuda()}
    out = {"P": P, "D": 45, "K": K, "flop_per_assign": 2.0 * P * K * 45}
    for name, x in data.items():
        c = x[torch.randperm(P, generator=torch.Generator().manual_seed(1))[:K].cuda()].contiguous()
        r = {}
        r["vq_assign"] = median_ms(lambda: dgr.vq_assign(x, c), a.warmup, a.steps)
        r["vq_assign"]["tflops"] = round(out["flop_per_assign"] / (r["vq_assign"]["ms"] * 1e-3) / 1e12, 2)
        r["vq_assign"]["of_f32_matrix_peak"] = round(r["vq_assign"]["tflops"] * 1e12 / F32_MATRIX_PEAK, 3)
        idx, _ = dgr.vq_assign(x, c)
        r["vq_update"] = median_ms(lambda: dgr.vq_update(x, idx, c), a.warmup, a.steps)
        keep, call = raw_update(x, idx.long(), c)
        r["msgs_vq_update_alone"] = median_ms(call, a.warmup, a.steps)
        if a.only == "all":
            r["torch_assign"] = median_ms(lambda: torch_assign(x, c, a.torch_rows), a.warmup, a.steps)
            r["torch_update"] = median_ms(lambda: torch_update(x, idx.long(), c), a.warmup, a.steps)
            r["agree_with_torch"] = round(float((torch_assign(x, c, a.torch_rows) == idx).float().mean()), 6)
            r["kmeans_10_iterations"] = {"ms": round(timed(lambda: compress.kmeans(x, K, iters=10, seed=0))[0], 2)}
        out[name] = r
        print(name, json.dumps(r), flush=True)
    if a.only == "all":
        with tempfile.TemporaryDirectory() as d:
            ply, npz = os.path.join(d, "model.ply"), os.path.join(d, "model.npz")
            model_io.save_ply(pc, ply)
            ms, _ = timed(lambda: compress.save_compressed(pc, npz, sh_codes=K, iters=10))
            report = compress.compressed_size_report(npz)
            out["save_compressed"] = {"ms": round(ms, 1), "ply_bytes": os.path.getsize(ply), "npz_bytes": report["total"],
                                      "fields": report}
        print("save_compressed", json.dumps(out["save_compressed"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
