"""The getters of the reference's GaussianModel (/root/reference/scene/gaussian_model.py:127-153) are what the op's chained mode has
to recognise in the autograd graph and what the raw-parameter entry evaluates inside its kernels.  Pinned here:
  * tests/golden/getters.npz + getter_graphs.json come from the reference's OWN class (make_getter_golden.py, build container):
    this repository's stand-in model must produce the same values bit for bit and the same autograd node chains;
  * _match_reference_getters must accept exactly that chain — including every saved argument it reads, which
    tests/golden/getter_graph_args.json records from the reference's own graphs (same generator) — and return the model's own
    leaf tensors."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
GOLD = np.load(os.path.join(HERE, "golden", "getters.npz"))
GRAPHS = json.load(open(os.path.join(HERE, "golden", "getter_graphs.json")))
GRAPH_ARGS = json.load(open(os.path.join(HERE, "golden", "getter_graph_args.json")))
LEAVES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
GETTERS = ("get_features", "get_opacity", "get_scaling", "get_rotation")


def _chain(t):
    out = []

    def rec(f, d):
        if f is None:
            return
        out.append([d, type(f).__name__])
        for nf, _ in f.next_functions:
            rec(nf, d + 1)
    rec(t.grad_fn, 0)
    return out


def _mirror():
    from synthetic_model import SyntheticGaussians
    m = object.__new__(SyntheticGaussians)
    for n in LEAVES:
        setattr(m, n, torch.nn.Parameter(torch.from_numpy(GOLD[n].copy())))
    return m


def test_stand_in_model_reproduces_the_reference_getters():
    m = _mirror()
    for name in GETTERS:
        got = getattr(m, name)
        assert np.array_equal(got.detach().numpy(), GOLD[name]), name
        assert _chain(got) == GRAPHS[name], name


def test_matcher_accepts_the_reference_chain():
    import diff_gaussian_rasterization as dgr
    m = _mirror()
    hit = dgr._match_reference_getters(m.get_xyz, m.get_features, m.get_opacity, m.get_scaling, m.get_rotation)
    assert hit is not None
    for t, n in zip(hit, LEAVES[1:]):
        assert t is getattr(m, n), n


def test_recorded_reference_getters_are_recognised():
    import diff_gaussian_rasterization as dgr
    from make_getter_golden import saved_args
    m = _mirror()
    leaves = {n: getattr(m, n) for n in LEAVES}
    for name in GETTERS:
        assert saved_args(getattr(m, name), leaves) == GRAPH_ARGS[name], name
    hit = dgr._match_reference_getters(m.get_xyz, m.get_features, m.get_opacity, m.get_scaling, m.get_rotation)
    assert hit is not None, "the op would not chain the reference's own getters"
    for t, n in zip(hit, LEAVES[1:]):
        assert t is getattr(m, n), n
