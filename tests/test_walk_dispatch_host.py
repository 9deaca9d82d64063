"""for_walk (molvoxel_amd/csrc/mvx_grad.h) without a GPU: the one place that turns a WalkKey (grid_kind, mode, gauss, chanwise)
into the template arguments of grad_kernel, grad_radii_kernel and score_kernel. Identical device code cannot show a key that
reaches the wrong instantiation; a small host program can: it calls for_walk for all 3 x 3 x 2 x 2 keys with a functor that
prints the tags it was given. No device pass: the header's dispatch is plain host C++."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "molvoxel_amd", "csrc")
MODE_FEATURES, MODE_TYPES, MODE_SINGLE = 0, 1, 2

PROGRAM = r"""
#include <cstdio>
#include <type_traits>
#include "mvx_grad.h"
using namespace mvx;
template <typename GT> const char *name() {
    static_assert(std::is_same<GT, float>::value || std::is_same<GT, __bf16>::value || std::is_same<GT, double>::value, "grid type");
    return std::is_same<GT, float>::value ? "float" : std::is_same<GT, __bf16>::value ? "bf16" : "double";
}
int main() {
    for (int grid_kind = 0; grid_kind < 3; ++grid_kind)
        for (int mode = 0; mode < 3; ++mode)
            for (int gauss = 0; gauss < 2; ++gauss)
                for (int chanwise = 0; chanwise < 2; ++chanwise) {
                    const WalkKey key{grid_kind, mode, gauss != 0, chanwise != 0};
                    const hipError_t e = for_walk(key, [&](auto gt, auto m, auto g, auto c) {
                        constexpr int M = decltype(m)::value;      // (the tags are compile-time constants)
                        constexpr bool G = decltype(g)::value, C = decltype(c)::value;
                        std::printf("%d %d %d %d -> %s %d %d %d\n", grid_kind, mode, gauss, chanwise,
                                    name<typename decltype(gt)::type>(), M, (int)G, (int)C);
                        return hipSuccess;
                    });
                    if (e != hipSuccess) return 1;
                }
    return 0;
}
"""


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_every_key_reaches_its_own_instantiation(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc: the header needs the HIP runtime's headers (hipError_t) even on the host")
    src, exe = tmp_path / "walk_dispatch.cpp", tmp_path / "walk_dispatch"
    src.write_text(PROGRAM)
    # -x c++: the host compiler alone, no device pass (so the HIP headers have to be named: <rocm>/bin/hipcc -> <rocm>/include)
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", rocm_include,
                           "-I", CSRC, str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    got = {}
    for line in lines:
        key, tags = line.split(" -> ")
        got[tuple(int(x) for x in key.split())] = tuple(tags.split())
    keys = list(itertools.product(range(3), range(3), range(2), range(2)))
    assert len(lines) == 36 and sorted(got) == keys  # every key called its functor exactly once
    for grid_kind, mode, gauss, chanwise in keys:
        gt, m, g, c = got[(grid_kind, mode, gauss, chanwise)]
        assert gt == ("float", "bf16", "double")[grid_kind]
        assert int(m) == (MODE_FEATURES if mode == MODE_FEATURES else MODE_TYPES)  # (single: type 0 in every record)
        assert int(g) == gauss
        assert int(c) == (1 if (mode == MODE_FEATURES and chanwise) else 0)
    assert len(set(got.values())) == 18  # 3 grid types x (features: 2 x 2, types / single: 2)
