"""The C++ shell's field functions (EvaluateField, ComposeDisplacements, SeedsFromField of host/Include/cRegistration.h) in one small
program, which tests/test_field_cpu.py runs without a GPU (every call fails and says so) and tests/test_gpu_field.py with one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHELL = r"""
#include <cstdio>
#include <vector>
#include "cRegistration.h"
int main() {
	std::vector<CPUSIFT::Cvec> pts;
	std::vector<CPUSIFT::IcgnResult> disp;
	for (int i = 0; i < 64; i++) {
		pts.push_back(CPUSIFT::Cvec((float)(4 * (i % 4)), (float)(4 * (i / 4 % 4)), (float)(4 * (i / 16))));
		CPUSIFT::IcgnResult r;
		r.status = 0;
		r.zncc = 0.99;
		r.p[0] = 0.5 + 0.01 * pts.back().x;
		r.p[1] = 0.01;
		disp.push_back(r);
	}
	CPUSIFT::FieldOptions o;
	o.radius = 8;
	const std::vector<double> x = {6.5, 6.25, 5.75, 100.0, 6.0, 6.0};
	std::vector<CPUSIFT::FieldResult> f = CPUSIFT::EvaluateField(pts, disp, x, o, 0.5);
	std::vector<CPUSIFT::FieldResult> moved = CPUSIFT::EvaluateField(pts, disp, pts, disp, o);
	std::vector<CPUSIFT::FieldResult> total = CPUSIFT::ComposeDisplacements(disp, moved);
	std::vector<CPUSIFT::AffineFit> seeds = CPUSIFT::SeedsFromField(pts, total);
	disp.pop_back();
	std::vector<CPUSIFT::FieldResult> bad = CPUSIFT::EvaluateField(pts, disp, x);
	std::vector<CPUSIFT::FieldResult> bad2 = CPUSIFT::ComposeDisplacements(disp, moved);
	std::printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d %.6f %.6f %.6f %d\n", f.size(), moved.size(), total.size(), seeds.size(), bad.size(),
	            f[0].status, f[1].status, moved[21].status, total[21].status, seeds[21].status, bad[0].status, f[0].disp[0], total[21].disp[0],
	            seeds[21].A[0], bad2[0].status);
	return 0;
}
"""


def run(tmp_path):
    """builds the program against the shell and the library and runs it: (the words it printed, its stderr)"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    d = os.path.join(ROOT, "3dsift_amd")
    if not os.path.exists(os.path.join(d, "libsift3d.so")):
        subprocess.check_call(["make", "-C", os.path.join(d, "host")])
    src = tmp_path / "field.cpp"
    src.write_text(SHELL)
    r = subprocess.run([cxx, "-std=c++14", "-Wall", "-Werror", "-o", str(tmp_path / "field"), str(src), "-I", os.path.join(d, "host", "Include"),
                        "-L" + d, "-lsift3d", "-lsift3d_hip", "-Wl,-rpath," + d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(tmp_path / "field")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.split(), r.stderr


def check_gpu_output(out):
    """u = 0.5 + 0.01 x on a 4 x 4 x 4 lattice of step 4: 0.565 at x = 6.5, and nothing within reach of x = 100; the point (4, 4, 4)
    moves to x = 4.54 where u_B = 0.5454, so the total is 1.0854 and 1 + G_xx = 1 + (0.01 + 0.01 + 0.0001); the calls with 63
    displacements fail"""
    assert out[:5] == ["2", "64", "64", "64", "2"], out
    assert out[5:11] == ["0", "1", "0", "0", "0", "-1"] and out[14] == "-1", out
    assert abs(float(out[11]) - 0.565) < 1e-6 and abs(float(out[12]) - 1.0854) < 1e-6 and abs(float(out[13]) - 1.0201) < 1e-6, out
