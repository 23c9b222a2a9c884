"""The wrapper's instance-count guess (diff_gaussian_rasterization._instance_guess / _note_instances / _capacity) and the capped
caches that hold it and the slab policy's statistics (_LRU).  The guess decides which route stage 2 of the forward takes:
speculative on buffers of _capacity(guess), or the redo on exact buffers when the view has more instances
(tests/test_stage2_routes_gpu.py)."""
import pytest

from route_utils import guesses_around, reset_forward_state


@pytest.fixture
def dgr():
    import diff_gaussian_rasterization as m
    reset_forward_state()
    yield m
    reset_forward_state()


def test_lru_evicts_the_least_recently_written_key_through_setitem(dgr):
    c = dgr._LRU(3)
    for k in "abc":
        c[k] = k
    c["a"] = "A"                     # re-written: most recent
    c["d"] = "d"
    assert list(c) == ["c", "a", "d"] and c["a"] == "A"
    for i in range(100):
        c[i] = i
    assert len(c) == 3 and list(c) == [97, 98, 99]


def test_lru_setdefault_keeps_the_cap(dgr):
    c = dgr._LRU(3)
    for i in range(10):
        v = c.setdefault(i, {"n": i})
        assert v == {"n": i} and v is c[i]
    assert len(c) == 3 and list(c) == [7, 8, 9]
    # an existing key: its value is returned (the same object, the stats dict the wrapper then updates) and nothing evicted
    d = c.setdefault(8, {"n": -1})
    assert d == {"n": 8} and d is c[8] and len(c) == 3 and 7 in c
    assert c.setdefault(10) is None and len(c) == 3 and 7 not in c


def test_feedback_stats_cache_is_capped(dgr):
    """_fb_stats is filled through setdefault (_note_info): its cap must hold"""
    for i in range(dgr._fb_stats.cap + 50):
        dgr._fb_stats.setdefault((0, i, 1, 0, 0), {})["D"] = i
    assert len(dgr._fb_stats) == dgr._fb_stats.cap
    assert (0, 49, 1, 0, 0) not in dgr._fb_stats and (0, dgr._fb_stats.cap + 49, 1, 0, 0) in dgr._fb_stats


def test_guess_of_a_known_key(dgr):
    key = (0, 1000, 640, 480, 0, 0)
    assert dgr._instance_guess(key) is None                        # nothing seen yet: the first-call route
    dgr._note_instances(key, 50_000, None)
    assert dgr._instance_guess(key) == 50_000
    # the key's own count wins over the view shape's
    dgr._instances_by_view[(0, 640, 480, 0, 0)] = (1, 1000)
    assert dgr._instance_guess(key) == 50_000


@pytest.mark.parametrize("P,expect", [(1010, 50_501), (800, 40_001), (1250, 62_501), (799, None), (1251, None),
                                      (1030, 51_501)])
def test_guess_from_the_view_shape_scales_with_P_within_the_gate(dgr, P, expect):
    """a key never seen (another model size) gets the last count of the same (device, W, H, filters), scaled by P, while
    0.8 <= P / P_last <= 1.25; another view shape or filter setting gets nothing"""
    dgr._note_instances((0, 1000, 640, 480, 0, 0), 50_000, None)
    assert dgr._instance_guess((0, P, 640, 480, 0, 0)) == expect
    assert dgr._instance_guess((0, P, 640, 481, 0, 0)) is None
    assert dgr._instance_guess((0, P, 640, 480, 1, 1)) is None
    assert dgr._instance_guess((1, P, 640, 480, 0, 0)) is None


def test_note_instances_halves_the_excess_toward_the_last_count(dgr):
    key = (0, 1000, 640, 480, 0, 0)
    dgr._note_instances(key, 10_000, None)
    assert dgr._last_instances[key] == 10_000
    # a smaller view: the guess comes down by half its excess per call, never below the count
    seq = []
    for _ in range(4):
        dgr._note_instances(key, 2_000, dgr._instance_guess(key))
        seq.append(dgr._last_instances[key])
    assert seq == [6_000, 4_000, 3_000, 2_500]
    # a larger count than the guess: taken at once
    dgr._note_instances(key, 30_000, dgr._instance_guess(key))
    assert dgr._last_instances[key] == 30_000
    assert dgr._instances_by_view[(0, 640, 480, 0, 0)] == (30_000, 1000)


def test_capacity_formula_and_its_boundary():
    import diff_gaussian_rasterization as dgr
    assert dgr._capacity(0) == 4096 and dgr._capacity(8) == 8 + 1 + 4096 and dgr._capacity(800_000) == 904_096
    for D in (4097, 4100, 5000, 123_457, 1_000_000, 1_000_001, 2_345_678, 40_000_003):
        below, fits = guesses_around(D)
        assert fits == below + 1
        assert dgr._capacity(below) < D <= dgr._capacity(fits), D
        assert all(dgr._capacity(g) < D for g in (below - 1, below // 2)) and dgr._capacity(10 * D) >= D
    # g + g // 8 skips values: some counts are met exactly by no guess, the smallest guess that fits then leaves room
    skipped = [D for D in range(4096 + 8, 4096 + 80) if dgr._capacity(guesses_around(D)[1]) != D]
    assert skipped
