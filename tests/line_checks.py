"""TEST INFRASTRUCTURE: what the checks of the two frame line estimators (tests/clock_checks.py, tests/fine_freq_checks.py;
csrc/frame_line.hpp) share."""
import irdm


def fill_with_cuts(out, fr, n):
    """`out` filled up to n frames with cuts of the frames `fr` at lengths and offsets of their own"""
    k = 0
    while len(out) < n:
        x = fr[k % len(fr)]
        off = 7 * k % 400
        out.append(x[off:off + 64 + (131 * k) % (len(x) - off - 64)])
        k += 1
    return out


def ragged3(n, block=32768):
    """n samples in three feeds of whole blocks, the remainder on the last"""
    b = n // block
    a, c = max(1, b // 5), max(1, b // 2)
    return [a * block, c * block, n - (a + c) * block]


def group_refuses(option):
    """a member of a group refuses the option, directly and through irdm_group_set_option"""
    g = irdm.Group(2_000_000, 1, max_chunk_samples=32768 * 8)
    try:
        L = irdm.lib()
        assert L.irdm_set_option(g.member(0), option, 1) == -1
        assert L.irdm_group_set_option(g.g, option, 1) == -1
    finally:
        g.close()
