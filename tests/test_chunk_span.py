"""The span geometry of the chunk passes (csrc/chunk_span.hpp) without a GPU: the host function chunk_span, compiled with
g++ against the HIP emulation's header, over every bytes-per-sample, every sample-aligned base within a 16-byte line and
the sample counts at which the head, the 16-byte pieces, the tail and the grid change -- against a brute-force restatement.

The five kernels that take a ChunkSpan (input_stats, iq_moments, iq_balance, iq_swap, scrub) index memory by nothing else:
16-byte loads at base + head * bps + 16 i for i < nvec, one sample per thread at the scalar indices.  The inequalities
asserted here are their bounds.
"""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "iridium-sniffer_amd", "csrc", "chunk_span.hpp")

SRC = r"""
#include "chunk_span.hpp"
extern "C" int span_of(int bps, unsigned long long addr, unsigned long long n, long long *out)
{
    int grid = -1;
    const irdm::ChunkSpan sp = irdm::chunk_span(bps, reinterpret_cast<const void *>(addr), (size_t)n, irdm::kChunkNT,
                                                irdm::kChunkMaxGrid, &grid);
    out[0] = sp.n;
    out[1] = sp.head;
    out[2] = sp.nvec;
    return grid;
}
extern "C" void span_constants(long long *out)
{
    out[0] = irdm::kChunkNT;
    out[1] = irdm::kChunkMaxGrid;
    out[2] = irdm::kChunkSlots;
    out[3] = (long long)irdm::kChunkMaxLaunch;
}
"""

NT, MAX_GRID = 256, 2048
COUNTS = list(range(41)) + [255, 256, 257, 1 << 31]
BASE = 0x7F0000001000          # a 4 KiB boundary, as an allocation's base


@pytest.fixture(scope="module")
def spanlib():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libchunkspan.so")
    src = os.path.join(out_dir, "chunk_span_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(HDR), os.path.getmtime(__file__)):
        with open(src, "w") as fh:
            fh.write(SRC)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "tests", "hip_emul"),
                               "-I", os.path.dirname(HDR), "-o", so, src])
    L = C.CDLL(so)
    L.span_of.argtypes = [C.c_int, C.c_ulonglong, C.c_ulonglong, C.POINTER(C.c_longlong)]
    L.span_constants.argtypes = [C.POINTER(C.c_longlong)]
    return L


def brute(bps, addr, n):
    """head: samples stepped over one by one until the address is a multiple of 16 or the samples are used up; nvec: whole
    16-byte pieces counted one by one (closed form past 4096 samples); grid: workgroups of NT threads counted likewise"""
    spv = 16 // bps
    head = 0
    while head < n and (addr + head * bps) % 16 != 0:
        head += 1
    left = n - head
    if left <= 4096:
        nvec = 0
        while (nvec + 1) * spv <= left:
            nvec += 1
    else:
        nvec = left // spv
    grid = 1
    while grid < MAX_GRID and grid * NT < nvec:
        grid += 1
    return head, nvec, grid


def test_constants(spanlib):
    out = (C.c_longlong * 4)()
    spanlib.span_constants(out)
    assert list(out) == [NT, MAX_GRID, 4, 1 << 31]


@pytest.mark.parametrize("bps", [2, 4, 8])
def test_chunk_span_against_brute_force(spanlib, bps):
    spv = 16 // bps
    out = (C.c_longlong * 3)()
    for off in range(0, 16, bps):
        addr = BASE + off
        for n in COUNTS:
            grid = spanlib.span_of(bps, addr, n, out)
            got_n, head, nvec = list(out)
            where = "bps %d offset %d n %d: head %d nvec %d grid %d" % (bps, off, n, head, nvec, grid)
            assert got_n == n, where
            assert (head, nvec, grid) == brute(bps, addr, n), where
            # the pieces and the scalar samples lie inside the chunk
            assert head >= 0 and nvec >= 0 and head + nvec * spv <= n, where
            # the head ends at the first boundary (or the chunk ends in front of it)
            assert head < spv or head == n, where
            # the tail is shorter than a piece
            tail = n - head - nvec * spv
            assert 0 <= tail < spv, where
            # 16-byte loads are aligned
            if nvec > 0:
                assert (addr + head * bps) % 16 == 0, where
            assert 1 <= grid <= MAX_GRID, where
            # the scalar samples fit the first workgroup, one per thread
            assert head + tail <= 2 * (spv - 1) <= NT, where
