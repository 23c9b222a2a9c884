"""`make isa` (tools/isa_mix.py on the emitted gfx950 assembly of blend.hip) still finds its kernels and writes every key
bench.py's roofline leg reads.  build() runs the target best-effort and bench.py falls back to a committed copy, so without
this test a renamed kernel or a changed template parameter list breaks the tool silently."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ms-gs_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # the Makefile's default
CLASSES = ("plain", "half", "trans", "salu", "lds", "vmem")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="no hipcc on this machine")
def test_make_isa_writes_what_bench_reads():
    r = subprocess.run(["make", "-C", PKG, "isa"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    isa = json.load(open(os.path.join(PKG, "build", "isa_mix.json")))
    assert set(isa["cycles_per_class"]) == set(CLASSES)
    fwd, bwd = isa["blend_fwd"], isa["blend_bwd"]
    for k in ("valu_per_wave_entry", "valu_cycles_per_wave_entry", "cycles_per_wave_entry"):
        assert fwd[k] > 0, k
    assert len(fwd["valu_mix"]) == 3 and abs(sum(fwd["valu_mix"]) - 1.0) < 1e-9
    for k in ("valu_per_quadrant_step", "valu_cycles_per_quadrant_step"):
        assert bwd[k] > 0, k
    for k in ("per_reduction", "per_entry_visit", "per_quadrant_step"):      # per_reduction: None when the tail was not found
        assert bwd[k] and set(bwd[k]) == set(CLASSES), k
        assert sum(bwd[k][c] for c in ("plain", "half", "trans")) > 0, k
