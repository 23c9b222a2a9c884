"""bench.py --dump-outputs without a GPU: dump_outputs() on CPU tensors shaped like one timed step's results (render() dict
plus the gradients on the leaves).  The files are float32, stay within 64 MB in all, keep the same seeded rows in every
per-Gaussian array and the same seeded pixels in every image plane, and are identical from one run to the next.  Runs in a child
process: importing bench.py sets process-wide torch options."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, types
import torch
sys.path.insert(0, sys.argv[1])
import bench
out_dir, P, H, W = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
idx = torch.arange(P, dtype=torch.float32)
pix = torch.arange(H * W, dtype=torch.float32).view(H, W)
viewspace = torch.zeros(P, 3)
viewspace.grad = idx[:, None].repeat(1, 3)
out = {"render": torch.stack([pix, pix + 0.25, pix + 0.5]), "acc_pixel_size": pix, "depth": -pix,
       "viewspace_points": viewspace, "visibility_filter": (torch.arange(P) % 3) == 0,
       "radii": torch.arange(P, dtype=torch.int32) % 97, "pixel_sizes": 0.5 * idx}
pc = types.SimpleNamespace(LEAVES=("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"))
shapes = ((P, 3), (P, 1, 3), (P, 15, 3), (P, 1), (P, 3), (P, 4))
params = []
for s in shapes:
    p = torch.zeros(s)
    p.grad = idx.view((P,) + (1,) * (len(s) - 1)).expand(s).contiguous()
    params.append(p)
pc.parameters = lambda: params
print(bench.dump_outputs(out_dir, out, pc, P, H, W))
"""

NAMES = {"render", "acc_pixel_size", "depth", "visibility_filter", "radii", "pixel_sizes", "viewspace_points_grad", "grad_xyz",
         "grad_features_dc", "grad_features_rest", "grad_opacity", "grad_scaling", "grad_rotation"}


def _dump(d, P, H, W):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(d), str(P), str(H), str(W)], capture_output=True, text=True,
                       timeout=600, cwd=str(d.parent))
    assert r.returncode == 0, r.stderr[-2000:]
    files = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert set(files) == NAMES
    assert all(a.dtype == np.float32 for a in files.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64_000_000
    return files


def _check_rows(f, P):
    rows = f["pixel_sizes"] / 0.5                       # every per-Gaussian array carries its row number
    assert np.array_equal(rows, np.round(rows)) and np.all(np.diff(rows) > 0) and rows.max() < P
    assert np.array_equal(f["radii"], rows % 97)
    assert np.array_equal(f["visibility_filter"], (rows % 3 == 0).astype(np.float32))
    for k in ("viewspace_points_grad", "grad_xyz", "grad_features_dc", "grad_features_rest", "grad_opacity", "grad_scaling",
              "grad_rotation"):
        assert f[k].shape[0] == rows.size and np.all(f[k] == rows.reshape((-1,) + (1,) * (f[k].ndim - 1))), k
    return rows


def test_small_step_is_written_whole(tmp_path):
    P, H, W = 1000, 48, 64
    f = _dump(tmp_path / "a", P, H, W)
    assert np.array_equal(_check_rows(f, P), np.arange(P))
    pix = np.arange(H * W, dtype=np.float32).reshape(H, W)
    assert np.array_equal(f["render"], np.stack([pix, pix + 0.25, pix + 0.5])) and np.array_equal(f["depth"], -pix)
    assert f["grad_features_rest"].shape == (P, 15, 3)


@pytest.mark.parametrize("P,H,W", [(1_000_000, 1080, 1920), (300_000, 2160, 3840)])
def test_large_step_is_sampled_within_the_limit_and_reproducible(tmp_path, P, H, W):
    f = _dump(tmp_path / "a", P, H, W)
    rows = _check_rows(f, P)
    assert rows.size == 1 << 16
    if H * W > 1920 * 1080:                             # 4K planes alone pass the limit: the same seeded pixels in each
        px = f["acc_pixel_size"]
        assert px.ndim == 1 and np.all(np.diff(px) > 0)
        assert np.array_equal(f["render"], np.stack([px, px + 0.25, px + 0.5])) and np.array_equal(f["depth"], -px)
    else:
        assert f["render"].shape == (3, H, W)
    g = _dump(tmp_path / "b", P, H, W)
    assert all(np.array_equal(f[k], g[k]) for k in NAMES)
