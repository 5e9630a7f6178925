"""CPU tests of the detection options' boundary (sift3d_set_detect_options, include/sift3d_hip.h): the header compiles as C and C++
with its layout guards, the library exports the entry points, the defaults need no GPU, and the C++ shell's extension methods link."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sift3d_default_detect_options", "sift3d_set_detect_options", "sift3d_get_detect_options", "sift3d_get_refined"]


@pytest.fixture(scope="module")
def capi():
    m = importlib.import_module("3dsift_amd.capi")
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "3dsift_amd", "csrc"), "-j8"])
    return m


PROBE = r"""
#include <stddef.h>
#include "sift3d_hip.h"
SIFT3D_STATIC_ASSERT(sizeof(sift3d_detect_options) == 32, "options");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_detect_options, reserved) == 20, "reserved");
SIFT3D_STATIC_ASSERT(sizeof(sift3d_refined) == 9 * sizeof(float), "refined");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_refined, contrast) == 32, "contrast");
int probe(sift3d_handle h) {
	sift3d_detect_options o;
	sift3d_refined r[1];
	sift3d_default_detect_options(&o);
	o.neighbours = 80;
	o.refine = 1;
	return sift3d_set_detect_options(h, &o) + sift3d_get_detect_options(h, &o) + sift3d_get_refined(h, r);
}
"""


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles(tmp_path, lang):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if not cc:
        pytest.skip("no host compiler")
    src = tmp_path / ("probe.c" if lang == "c" else "probe.cpp")
    src.write_text(PROBE)
    std = "-std=c11" if lang == "c" else "-std=c++14"
    r = subprocess.run([cc, std, "-Wall", "-Werror", "-c", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "probe.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_exports(capi):
    L = capi.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in capi.SYMBOLS


def test_defaults_without_gpu(capi):
    o = capi.DetectOptions()
    C.memset(C.byref(o), 0x5A, C.sizeof(o))
    capi.lib().sift3d_default_detect_options(C.byref(o))
    assert (o.neighbours, o.refine, o.max_offset, o.contrast_thresh, o.edge_ratio) == (8, 0, 0.5, 0.0, 0.0)
    assert list(o.reserved) == [0, 0, 0]
    assert capi.default_detect_options() == {"neighbours": 8, "refine": False, "max_offset": 0.5, "contrast_thresh": 0.0, "edge_ratio": 0.0}
    assert capi.REFINED_DTYPE.itemsize == 36 and capi.REFINED_DTYPE.fields["contrast"][1] == 32
    # a null handle is refused, not dereferenced
    assert capi.lib().sift3d_set_detect_options(None, C.byref(o)) == 1
    assert capi.lib().sift3d_get_refined(None, None) == 1


SHELL = r"""
#include <vector>
#include "cSIFT3D.h"
int main() {
	CPUSIFT::CSIFT3D *s = CPUSIFT::CSIFT3DFactory::CreateCSIFT3D(nullptr, 0, 0, 0);
	CPUSIFT::CSIFT3D::DetectOptions o;
	o.neighbours = 80;
	o.refine = 1;
	o.edge_ratio = 10.0f;
	bool ok = s && s->SetDetectOptions(o);
	if (s) s->KpSiftAlgorithm();
	std::vector<CPUSIFT::Cvec> rc = s ? s->GetRefinedCoordinates() : std::vector<CPUSIFT::Cvec>();
	std::vector<float> sc = s ? s->GetRefinedScales() : std::vector<float>();
	delete s;
	return ok ? (int)(rc.size() + sc.size()) : 1;
}
"""


def test_shell_extension_links(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    lib = os.path.join(ROOT, "3dsift_amd", "libsift3d.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "3dsift_amd", "host")])
    src = tmp_path / "shell.cpp"
    src.write_text(SHELL)
    d = os.path.join(ROOT, "3dsift_amd")
    r = subprocess.run([cxx, "-std=c++14", "-Wall", "-o", str(tmp_path / "shell"), str(src), "-I", os.path.join(d, "host", "Include"),
                        "-L" + d, "-lsift3d", "-lsift3d_hip", "-Wl,-rpath," + d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
