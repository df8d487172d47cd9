"""CPU: the partition rule of the EVEN list walk (cips_siren_bwd_x3_live_plan_host, the host evaluation of the function
the plan kernel runs on the device; include/cips3d_hip.h has the rule).  The SIREN backward trusts the table for its list
reads, so everything it relies on is checked here, on the host, before any kernel sees a table: the budget, the cover of
every image's list, the balance inside an image and across images, and the idle ids."""
import ctypes as C

import numpy as np
import pytest


def _lib():
    from cips3d_amd import _lib
    return _lib.load()


def plan(count, P):
    """-> seg (G, 4), img (B, 2), G, chunks"""
    lib = _lib()
    count = np.ascontiguousarray(count, dtype=np.int32)
    B = len(count)
    chunks = lib.cips_siren_bwd_x3_chunks(B, P)
    G = B * chunks
    seg = np.full((G, 4), -7, dtype=np.int32)
    img = np.full((B, 2), -7, dtype=np.int32)
    rc = lib.cips_siren_bwd_x3_live_plan_host(count.ctypes.data_as(C.c_void_p), B, P, seg.ctypes.data_as(C.c_void_p),
                                              img.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return seg, img, G, chunks


def rule_T(count, G):
    """T of the rule, by its definition (a linear search from the lower bound)"""
    r = [-(-int(c) // 128) for c in count]
    T = max(1, -(-sum(r) // G))
    while sum(max(1, -(-x // T)) for x in r) > G:
        T += 1
        assert T <= max(r)
    return T


def check_plan(count, P):
    seg, img, G, _ = plan(count, P)
    B = len(count)
    r = [-(-int(c) // 128) for c in count]
    T = rule_T(count, G)
    n = img[:, 1]
    assert (n >= 1).all() and int(n.sum()) <= G
    assert [int(x) for x in n] == [max(1, -(-x // T)) for x in r]
    assert img[:, 0].tolist() == [int(n[:b].sum()) for b in range(B)]
    used = int(n.sum())
    for b in range(B):
        rows = seg[img[b, 0]:img[b, 0] + n[b]]
        assert (rows[:, 0] == b).all()
        pos = 0
        for j, (_, first, end, nr) in enumerate(rows.tolist()):
            assert first == pos and first % 128 == 0                       # contiguous from 0, whole rounds
            assert end == min(first + nr * 128, int(count[b]))             # ... except a clipped end
            assert (end - first + 127) // 128 == nr
            pos = first + nr * 128
        assert rows[-1, 2] == count[b] and int(rows[:, 3].sum()) == r[b]   # covers [0, count_b) exactly once
        assert int(rows[:, 3].max()) - int(rows[:, 3].min()) <= 1
        assert (np.diff(rows[:, 3]) <= 0).all()                            # the longer workgroups come first
        assert count[b] == 0 or int(rows[:, 3].min()) >= 1
    assert int(seg[:used, 3].max()) <= T
    assert (seg[used:] == np.array([-1, 0, 0, 0])).all()                   # idle ids
    return seg, img, G, T


def test_equal_counts_give_the_dense_partition():
    """b = 2, P = 1024: two workgroups of 512 slots per image in row order b * chunks + c; b = 32, P = 98304 (the headline
    shape: 24 workgroups per image) with every count the same multiple of 24 * 128"""
    seg, img, G, T = check_plan([1024, 1024], 1024)
    assert G == 4 and T == 4
    assert seg.tolist() == [[0, 0, 512, 4], [0, 512, 1024, 4], [1, 0, 512, 4], [1, 512, 1024, 4]]
    assert img.tolist() == [[0, 2], [2, 2]]
    for cnt in (98304, 24 * 128 * 19):
        seg, img, G, T = check_plan([cnt] * 32, 98304)
        assert G == 768 and T == cnt // (24 * 128)
        ln = cnt // 24
        want = [[b, c * ln, (c + 1) * ln, T] for b in range(32) for c in range(24)]
        assert seg.tolist() == want
        assert img.tolist() == [[24 * b, 24] for b in range(32)]


def test_one_full_image_takes_the_idle_workgroups_of_the_empty_ones():
    P = 98304
    count = [0] * 32
    count[5] = P
    seg, img, G, T = check_plan(count, P)
    chunks = G // 32
    assert T == 2 and img[5].tolist() == [5, 384] and img[5, 1] > 10 * chunks     # 768 rounds over 768 - 31 workgroups
    for b in range(32):
        if b != 5:
            assert img[b, 1] == 1 and seg[img[b, 0]].tolist() == [b, 0, 0, 0]
    assert int((seg[:, 0] == -1).sum()) == G - 384 - 31


def test_the_skewed_case_of_the_gpu_test():
    """b = 4, P = 2048 (chunk 512, G = 16): counts 2048, 384, 5, 0 -> T = 2, n = [8, 2, 1, 1], 4 idle ids"""
    seg, img, G, T = check_plan([2048, 3 * 128, 5, 0], 2048)
    assert G == 16 and T == 2
    assert img[:, 1].tolist() == [8, 2, 1, 1]
    assert seg[8:12].tolist() == [[1, 0, 256, 2], [1, 256, 384, 1], [2, 0, 5, 1], [3, 0, 0, 0]]
    assert (seg[12:, 0] == -1).all()


def test_all_zero_one_image_and_ragged():
    seg, img, G, T = check_plan([0, 0, 0], 128 * 7 + 5)
    assert T == 1 and img.tolist() == [[0, 1], [1, 1], [2, 1]]
    assert seg[:3].tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0]]
    P = 128 * 7 + 5                                       # count = P, not a multiple of 128: the last round is clipped
    seg, img, G, T = check_plan([P], P)
    assert img.tolist() == [[0, G]] and seg[-1, 2] == P
    check_plan([P, P, P], P)
    check_plan([1], 1)
    check_plan([77], 98304 * 8)


def test_random_counts():
    rng = np.random.default_rng(7)
    for B, P in [(32, 98304), (3, 128 * 7 + 5), (4, 2048), (1, 5000), (7, 40000), (64, 98304), (5, 300)]:
        for k in range(6):
            if k == 0:
                count = rng.integers(0, P + 1, B)
            elif k == 1:                                   # shares spread like the recorded ones, 0.18 .. 0.99
                count = (np.clip(rng.normal(0.6, 0.22, B), 0.05, 0.99) * P).astype(np.int64)
            elif k == 2:                                   # most images empty
                count = np.where(rng.random(B) < 0.7, 0, rng.integers(0, P + 1, B))
            elif k == 3:                                   # around the round boundaries
                count = np.minimum(P, 128 * rng.integers(0, P // 128 + 1, B) + rng.integers(-1, 2, B)).clip(0)
            elif k == 4:
                count = np.full(B, P)
            else:
                count = rng.integers(0, 3, B)
            check_plan(count, P)


def test_counts_out_of_range_are_clamped_and_arguments_validated():
    """a count above P (or negative) cannot send a range past the list; NULL tables are refused"""
    seg = plan([5000, -3], 1024)[0]
    assert seg[:, 0].tolist() == [0, 0, 0, 1] and seg[3].tolist() == [1, 0, 0, 0]        # 8 rounds, 0 rounds: T = 3
    assert int(seg[:, 2].max()) == 1024 and int(seg[:, 1].min()) == 0
    lib = _lib()
    buf = (C.c_int * 8)()
    assert lib.cips_siren_bwd_x3_live_plan_host(None, 1, 128, buf, buf) == 1
    assert lib.cips_siren_bwd_x3_live_plan_host(buf, 0, 128, buf, buf) == 1
    assert lib.cips_siren_bwd_x3_live_plan_host(buf, 1, 128, None, buf) == 1
    assert lib.cips_siren_bwd_x3_live_plan(None, 1, 128, buf, buf, None) == 1
    assert lib.cips_siren_bwd_x3_live_plan(buf, 1, 0, buf, buf, None) == 1
    assert lib.cips_siren_bwd_x3_reduce_segments(None, buf, buf, 1, buf, buf, None) == 1
    assert lib.cips_siren_bwd_x3_live_even(None, None, None, None, None, None, None, None, None, 1, 128, None) == 1
    assert lib.cips_siren_bwd_x3_rays_live_even(None, None, None, None, None, None, None, None, None, 1, None) == 1
