"""CPU checks of the depth-gradient entry points (include/msgs.h: msgs_backward_with_depth and its verification-mode scratch
query): declared, exported by the built library, listed in the ctypes surface, ABI version unchanged."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msgs_backward_with_depth", "msgs_backward_scratch_bytes_deterministic_depth")


def test_header_declares_depth_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msgs.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n


def test_library_exports_and_lists_them():
    import diff_gaussian_rasterization as dgr
    for n in NEW:
        assert hasattr(dgr._C.lib, n), n
        assert n in dgr._C.EXPORTS, n
    assert dgr._C.lib.msgs_abi_version() == 11


def test_depth_scratch_query_is_its_own():
    """the verification mode's depth layout holds ten sums per tile entry; the colour-only query is unchanged by it"""
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    P, D = 1000, 100000
    colour, depth = lib.msgs_backward_scratch_bytes_deterministic(P, D), lib.msgs_backward_scratch_bytes_deterministic_depth(P, D)
    assert depth >= colour + 8 * D
    assert lib.msgs_backward_scratch_bytes_deterministic(P, D) == colour
