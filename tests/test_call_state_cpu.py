"""The scratch layout of the one-shot entry points (3dsift_amd/csrc/scratch_layout.h), checked by a stand-alone host program
that includes nothing but that header and is built with the address and undefined-behaviour sanitizers: the properties every layout
relies on, over random size sequences, and two real layouts replayed against the offset chains the entries used to spell out."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dsift_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "scratch_layout.h"

#define CHECK(c) do { if (!(c)) { printf("line %d: %s (sequence %d)\n", __LINE__, #c, seq); return 1; } } while (0)

int main(int argc, char **argv) {
	int seq = -1;
	if (argc > 1) {  // replay: the sizes of the pieces -> their offsets, then the end
		s3d::Layout L;
		for (int i = 1; i < argc; i++) printf("%zu ", L.take(strtoull(argv[i], nullptr, 10)));
		printf("%zu\n", L.end);
		return 0;
	}
	unsigned long long x = 88172645463325252ull;
	auto rnd = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
	for (seq = 0; seq < 400; seq++) {
		s3d::Layout L;
		std::vector<size_t> at, bytes;
		const int pieces = 1 + (int)(rnd() % 12);
		for (int i = 0; i < pieces; i++) {
			const unsigned long long kind = rnd() % 4;  // zeros, sizes about a multiple of 256, small and large ones
			const size_t b = kind == 0 ? 0 : kind == 1 ? 256 * (1 + rnd() % 9) + rnd() % 3 - 1 : kind == 2 ? rnd() % 700 : rnd() % ((size_t)5 << 30);
			const size_t before = L.end, o = L.take(b);
			CHECK(o == before && o % 256 == 0 && L.end % 256 == 0);
			CHECK(b != 0 || L.end == before);  // take(0) does not advance
			CHECK(L.end >= o + b && L.end - (o + b) < 256);
			at.push_back(o);
			bytes.push_back(b);
		}
		for (int i = 0; i < pieces; i++)
			for (int j = i + 1; j < pieces; j++) CHECK(at[i] + bytes[i] <= at[j]);  // pieces in the order taken, none overlaps a later one
		CHECK(L.end >= at.back() + bytes.back());
	}
	printf("ok %d\n", seq);
	return 0;
}
"""


@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    t = tmp_path_factory.mktemp("layout")
    src, exe = os.path.join(t, "layout_check.cpp"), os.path.join(t, "layout_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, "-o", exe, src])
    return exe


def _replay(exe, sizes):
    out = subprocess.run([exe] + [str(s) for s in sizes], capture_output=True, text=True, check=True, timeout=60).stdout.split()
    return [int(v) for v in out[:-1]], int(out[-1])


def _al256(b):
    return (b + 255) & ~255


def test_random_sequences(layout_check):
    r = subprocess.run([layout_check], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 400", r.stdout + r.stderr


def test_icgn_host_inputs_layout(layout_check):
    # sift3d_icgn, host inputs with init: [results m | state m | ref | tar | points | init]; m = 10 POIs, ref 20^3, tar 21 x 20 x 19 voxels,
    # 128-byte result records, 1368-byte state records (IcgnState: 170 doubles, a float and an int)
    m, nr, nt, res, state = 10, 20 * 20 * 20, 21 * 20 * 19, 128, 1368
    sizes = [res * m, state * m, 4 * nr, 4 * nt, 4 * 3 * m, 8 * 12 * m]
    at, end = _replay(layout_check, sizes)
    # the entry's former chain: o_state = al256(res_bytes), o_ref = o_state + al256(state m), o_tar = o_ref + al256(4 nr), ...
    o_state = _al256(res * m)
    o_ref = o_state + _al256(state * m)
    o_tar = o_ref + _al256(4 * nr)
    o_pts = o_tar + _al256(4 * nt)
    o_init = o_pts + _al256(4 * 3 * m)
    assert at == [0, o_state, o_ref, o_tar, o_pts, o_init] == [0, 1280, 15104, 47104, 79104, 79360]
    assert end == 80384 and 0 <= end - (o_init + 8 * 12 * m) < 256  # (the former size ended at the last byte of init: 80320)
    # without init the last piece takes no room and keeps its offset
    at0, end0 = _replay(layout_check, sizes[:-1] + [0])
    assert at0 == at and end0 == o_init


def test_global_fit_layout(layout_check):
    # sift3d_fit_affine, host inputs: [fit | mask n | hyp 12 H doubles | count H ints | pairs 6 n floats]; n = 100 pairs, H = 4096
    # hypotheses, a 224-byte fit record; the pinned block is [fit | mask] = the offset of hyp
    n, H, fit = 100, 4096, 224
    at, end = _replay(layout_check, [fit, n, 8 * 12 * H, 4 * H, 4 * 6 * n])
    o_mask = _al256(fit)
    o_hyp = o_mask + _al256(n)
    o_cnt = o_hyp + _al256(8 * 12 * H)
    o_pairs = o_cnt + _al256(4 * H)
    assert at == [0, o_mask, o_hyp, o_cnt, o_pairs] == [0, 256, 512, 393728, 410112]
    assert end == 412672 and 0 <= end - (o_pairs + 4 * 6 * n) < 256  # (formerly 412512)
    # device inputs: no room for the pairs
    at_dev, end_dev = _replay(layout_check, [fit, n, 8 * 12 * H, 4 * H, 0])
    assert at_dev == at and end_dev == o_pairs
