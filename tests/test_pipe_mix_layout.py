"""RV_OPT_PIPE_MIX's dispatch layout (include/rvgrt/rv_internal.h pipe_layout / pipe_map, the function
k_ref_pipe calls), evaluated on the host through rv_pipe_layout_map: over the workgroups of a launch every
(part, part-local workgroup) appears exactly once, a workgroup keeps its position in its row of 8 (the XCD
it runs on), every part keeps its own order, and pattern 0 is the three contiguous ranges.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

ROWS = (0, 8, 16, 24, 40, 4096)          # part lengths in rows of 8 workgroups
ORDERS = (0x012, 0x021, 0x102, 0x120, 0x201, 0x210)
PATTERNS = ((1, 0, 4), (1, 0, 3), (1, 0, 2), (1, 1, 4))   # r_pp, r_gi, r_render of the A/B
# the second A/B round (profiles/r07/pipe_mix_ab.txt); 3:2:12 is the default
MORE = ((3, 2, 12), (2, 1, 8), (2, 0, 8), (2, 1, 7), (2, 1, 9), (2, 2, 8), (3, 1, 12), (4, 1, 16), (4, 2, 16), (2, 1, 10),
        (1, 1, 6), (3, 1, 11), (3, 1, 13), (5, 2, 20), (1, 1, 3), (1, 1, 5), (1, 0, 6), (1, 1, 2))
GI, PP, RENDER = 0, 1, 2


def pack(head, pat):
    return head << 24 | pat[0] << 16 | pat[1] << 8 | pat[2]


@pytest.fixture(scope="module")
def lib():
    import rvgrt_amd
    return rvgrt_amd._lib.load()


def layout(lib, order, mix, lens):
    n = int(sum(lens))
    part = np.full(n + 1, 255, np.uint8)
    local = np.full(n + 1, 0xFFFFFFFF, np.uint32)
    la = (C.c_uint32 * 3)(*lens)
    assert lib.rv_pipe_layout_map(order, mix, la, 0, n, part.ctypes.data, local.ctypes.data) == 0
    assert part[n] == 255 and local[n] == 0xFFFFFFFF   # nothing written past n
    return part[:n], local[:n]


def check(part, local, lens):
    n = len(part)
    b = np.arange(n, dtype=np.uint32)
    assert np.array_equal(local & 7, b & 7)
    for q in range(3):
        mine = local[part == q]
        # exactly once, and in the part's own order (its SCHED_COST order: ascending part-local rows)
        assert np.array_equal(mine, np.arange(lens[q], dtype=np.uint32)), q
    assert (part <= 2).all()


@pytest.mark.parametrize("order", ORDERS)
def test_pattern_zero_is_three_contiguous_ranges(lib, order):
    seq = [(order >> 8) & 15, (order >> 4) & 15, order & 15]
    for rows in itertools.product(ROWS, repeat=3):
        lens = [8 * v for v in rows]
        part, local = layout(lib, order, 0, lens)
        want_p = np.concatenate([np.full(lens[q], q, np.uint8) for q in seq])
        want_l = np.concatenate([np.arange(lens[q], dtype=np.uint32) for q in seq])
        assert np.array_equal(part, want_p) and np.array_equal(local, want_l), (order, rows)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("pat", PATTERNS)
def test_every_workgroup_once(lib, order, pat):
    for rows in itertools.product(ROWS, repeat=3):
        lens = [8 * v for v in rows]
        for head in (0, 1, rows[PP] // 8, rows[PP] // 4, rows[PP] + 5):
            part, local = layout(lib, order, pack(head, pat), lens)
            check(part, local, lens)
            h = min(head, rows[PP])
            assert (part[:8 * h] == PP).all()                      # the head: pre-pass rows first


@pytest.mark.parametrize("order", (0x102, 0x210))
def test_every_workgroup_once_second_round(lib, order):
    for pat in MORE:
        for rows in itertools.product(ROWS, repeat=3):
            lens = [8 * v for v in rows]
            for head in (0, 1, rows[PP] + 5):
                part, local = layout(lib, order, pack(head, pat), lens)
                check(part, local, lens)


def test_pattern_shape(lib):
    """1:0:4 with a head of 2 rows, order pre-pass, GI, render: head, the GI range, then 1 pre-pass row to 4
    render rows until the pre-pass runs out, the render ending contiguous."""
    lens = [8 * 3, 8 * 5, 8 * 40]   # GI, pre-pass, render
    part, local = layout(lib, 0x102, pack(2, (1, 0, 4)), lens)
    rows = part.reshape(-1, 8)
    assert (rows == rows[:, :1]).all()
    got = "".join("GPR"[v] for v in rows[:, 0])
    assert got == "PP" + "GGG" + "PRRRR" * 3 + "R" * 28
    check(part, local, lens)
    # 1:1:4, no head, a GI part shorter than the pre-pass: it drops out and the rest goes on
    part, local = layout(lib, 0x102, pack(0, (1, 1, 4)), [8 * 2, 8 * 4, 8 * 24])
    got = "".join("GPR"[v] for v in part.reshape(-1, 8)[:, 0])
    assert got == "PGRRRR" * 2 + "PRRRR" * 2 + "R" * 8
    # a part short of its share of a period: its last rows follow as one range
    part, local = layout(lib, 0x102, pack(0, (1, 0, 4)), [0, 8 * 3, 8 * 10])
    got = "".join("GPR"[v] for v in part.reshape(-1, 8)[:, 0])
    assert got == "PRRRR" * 2 + "RR" + "P"


def test_zero_length_parts(lib):
    """The last launch of a call without carry renders only: GI and pre-pass of length 0."""
    for pat in PATTERNS:
        for head in (0, 1, 7):
            part, local = layout(lib, 0x102, pack(head, pat), [0, 0, 8 * 24])
            assert (part == RENDER).all() and np.array_equal(local, np.arange(8 * 24, dtype=np.uint32))
    part, _ = layout(lib, 0x102, pack(3, (1, 1, 4)), [0, 0, 0])
    assert len(part) == 0


def test_large_launch_and_odd_ratios(lib):
    """C4-sized parts and ratios up to 255: the multiply-high division is exact for every row."""
    lens = [8 * 512, 8 * 4080, 8 * 16320]
    for pat, head in (((1, 0, 4), 510), ((3, 2, 7), 1020), ((255, 1, 255), 0), ((2, 255, 5), 33)):
        part, local = layout(lib, 0x102, pack(head, pat), lens)
        check(part, local, lens)


def test_refused_arguments(lib):
    la = (C.c_uint32 * 3)(8, 8, 8)
    out_p, out_l = np.zeros(24, np.uint8), np.zeros(24, np.uint32)
    f = lib.rv_pipe_layout_map
    assert f(0x112, 0, la, 0, 24, out_p.ctypes.data, out_l.ctypes.data) != 0    # not a permutation
    assert f(0x102, -1, la, 0, 24, out_p.ctypes.data, out_l.ctypes.data) != 0
    assert f(0x102, 0, (C.c_uint32 * 3)(8, 12, 8), 0, 24, out_p.ctypes.data, out_l.ctypes.data) != 0
    assert f(0x102, 0, la, 0, 24, None, out_l.ctypes.data) != 0
