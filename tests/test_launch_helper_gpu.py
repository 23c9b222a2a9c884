"""The Python op's shared plumbing (diff_gaussian_rasterization/__init__.py): _launch, the one way an entry point outside the
step's hot path is called, _stream and the device check _require_hip.  No kernel is launched here: msgs_contrib_finish returns in
front of every pointer for P == 0 (MSGS_OK) and P < 0 (MSGS_ERR_INVALID_ARG, which _C.check turns into ValueError)."""
import re

import pytest
import torch

import diff_gaussian_rasterization as dgr

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _finish(probe, P):
    return dgr._launch(probe, "msgs_contrib_finish", _dev(), P, None, 0, None, None, None)


def test_launch_runs_the_probe_then_the_entry():
    calls = []
    assert _finish(calls.append, 0) is None
    assert calls == ["msgs_contrib_finish"]


def test_launch_probes_before_the_call_and_names_the_entry_in_its_error():
    calls = []
    with pytest.raises(ValueError) as e:
        _finish(calls.append, -1)
    assert str(e.value).startswith("msgs_contrib_finish:")
    assert calls == ["msgs_contrib_finish"]


def test_launch_without_a_probe():
    assert _finish(None, 0) is None
    with pytest.raises(ValueError, match=r"^msgs_contrib_finish:"):
        _finish(None, -1)


def test_stream_is_the_current_stream_of_the_device():
    dev = _dev()
    # (the default stream's handle is 0, which a c_void_p reads back as None: compare as integers)
    assert (dgr._stream(dev).value or 0) == torch.cuda.current_stream(dev).cuda_stream
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):      # a cached or default stream would be caught here
        assert side.cuda_stream != 0
        assert dgr._stream(dev).value == torch.cuda.current_stream(dev).cuda_stream == side.cuda_stream
    assert (dgr._stream(dev).value or 0) == torch.cuda.current_stream(dev).cuda_stream


def test_require_hip():
    with pytest.raises(RuntimeError) as e:
        dgr._require_hip("f", x=torch.zeros(1))
    assert str(e.value) == "f: x must live on a HIP device ('cuda'); there is no CPU path"
    with pytest.raises(RuntimeError) as e:
        dgr._require_hip("f", ("the volume", torch.device("cpu")))
    assert str(e.value) == "f: the volume must live on a HIP device ('cuda'); there is no CPU path"
    dev = _dev()
    x, y = torch.zeros(1, device=dev), torch.zeros(2, device=dev)
    assert dgr._require_hip("f", x=x, none=None, y=y) == dev
    assert dgr._require_hip("f", ("the volume", dev), x=x) == dev
    if torch.cuda.device_count() >= 2:
        other = torch.device("cuda", (dev.index + 1) % torch.cuda.device_count())
        z = torch.zeros(1, device=other)
        with pytest.raises(ValueError, match=re.escape(f"f: z is on {other}, x on {dev}")):
            dgr._require_hip("f", x=x, z=z)
        with pytest.raises(ValueError, match=re.escape(f"f: z is on {other}, the volume on {dev}")):
            dgr._require_hip("f", ("the volume", dev), z=z)
