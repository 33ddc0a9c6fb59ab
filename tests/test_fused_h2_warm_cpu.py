"""CPU: the share arithmetic of the fused fp16x2 step's L2 warm-up (csrc/h2_warm.h, which mlp_fused_step_h2_kernel includes),
compiled as a host program: for every blockIdx.x in 0 .. 1023 the 256 threads of a workgroup read one dword of every 128-byte line
of ONE share of a weight plane, shares 0 .. 31 cover each plane exactly (no line twice, none left out), the share is
(blockIdx.x >> 3) & 31, and no byte offset reaches past the plane.  Also at a plane size and a workgroup size that are no multiples
of anything (several loads per thread, a short last share, a plane that ends inside its last line)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <set>
#include "flyhip.h"
#include "h2_warm.h"
int main(int argc, char** argv)
{
    // argv: plane bytes (0: the PH plane, 1: the PTH plane), threads per workgroup
    unsigned bytes = (unsigned)std::strtoul(argv[1], nullptr, 10);
    const unsigned threads = (unsigned)std::strtoul(argv[2], nullptr, 10);
    if (bytes == 0) bytes = 2u * MLP_PH_HALVES_ABI;
    if (bytes == 1) bytes = 2u * MLP_PTH_HALVES_ABI;
    std::printf("plane %u %u %u %u\n", bytes, h2_warm_lines(bytes), h2_warm_share_lines(bytes), h2_warm_loads(bytes, threads));
    for (unsigned block = 0; block < 1024; ++block) {
        const unsigned share = h2_warm_share(block);
        std::set<unsigned> lines;
        unsigned maxoff = 0, misaligned = 0;
        for (unsigned j = 0; j < h2_warm_loads(bytes, threads); ++j)
            for (unsigned t = 0; t < threads; ++t) {
                const unsigned off = h2_warm_offset(bytes, share, j, t, threads);
                lines.insert(off / H2_WARM_LINE);
                if (off > maxoff) maxoff = off;
                misaligned |= off & 3u;
            }
        const unsigned first = *lines.begin(), last = *lines.rbegin();
        std::printf("block %u %u %u %u %u %u %u\n", block, share, first, (unsigned)lines.size(), last - first + 1 == lines.size(), maxoff, misaligned);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("h2_warm")
    src = d / "h2_warm_shares.cpp"
    src.write_text(SRC)
    cxx = shutil.which("g++")
    cmd = [cxx] if cxx else [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]
    exe = str(d / "h2_warm_shares")
    subprocess.check_call(cmd + ["-std=c++17", "-I", os.path.join(REPO, "include"),
                                 "-I", os.path.join(REPO, "fly_bproject_amd", "csrc"), str(src), "-o", exe])
    return exe


def _run(program, bytes_arg, threads):
    out = subprocess.run([program, str(bytes_arg), str(threads)], capture_output=True, text=True, check=True).stdout.split("\n")
    head = out[0].split()
    assert head[0] == "plane"
    nbytes, lines, per, loads = (int(v) for v in head[1:])
    blocks = [[int(v) for v in line.split()[1:]] for line in out[1:] if line]
    assert [b[0] for b in blocks] == list(range(1024))
    return nbytes, lines, per, loads, blocks


def _check(nbytes, lines, blocks):
    by_share = {}
    for block, share, first, n, contiguous, maxoff, misaligned in blocks:
        assert share == (block >> 3) & 31, block
        assert contiguous == 1 and misaligned == 0, block
        assert maxoff + 4 <= nbytes, (block, maxoff, nbytes)                # no byte of a load reaches past the plane
        assert by_share.setdefault(share, (first, n)) == (first, n), (block, "two workgroups of one share read different lines")
    assert sorted(by_share) == list(range(32))
    nxt = 0
    for share in range(32):                                                 # shares 0 .. 31 tile the plane's lines: no gap, no overlap
        first, n = by_share[share]
        if nxt < lines:
            assert first == nxt and n >= 1, (share, first, nxt)
            nxt = first + n
        else:                                                               # (an empty share re-reads the last line)
            assert (first, n) == (lines - 1, 1), share
    assert nxt == lines


@pytest.mark.parametrize("plane", [0, 1], ids=["PH", "PTH"])
def test_the_32_shares_cover_a_weight_plane_exactly_and_stay_inside_it(program, plane):
    from fly_bproject_amd import policy as P
    nbytes, lines, per, loads, blocks = _run(program, plane, 256)
    assert nbytes == 2 * (P.LAYOUT.ph_halves, P.LAYOUT.pth_halves)[plane]
    assert nbytes % 128 == 0 and lines == 32 * per and loads == 1           # what the kernel's static_assert relies on: one load per thread
    _check(nbytes, lines, blocks)


@pytest.mark.parametrize("nbytes,threads", [(128 * 1000 + 36, 7), (128 * 31, 256), (4, 64), (128 * 33 - 4, 1)])
def test_odd_plane_and_workgroup_sizes_are_covered_and_clamped(program, nbytes, threads):
    got, lines, per, loads, blocks = _run(program, nbytes, threads)
    assert got == nbytes and lines == (nbytes + 127) // 128 and per * 32 >= lines and loads * threads >= per
    _check(nbytes, lines, blocks)
