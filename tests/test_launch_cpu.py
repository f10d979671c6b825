"""grid_for and with_lpp (aix_launch.hpp: the grid of the flat grid-stride kernels and the lanes-per-bucket dispatch) on the host: a small
program built with the project's hipcc, host side only, run as a fresh process per setting of AIX_GRID_PER_CU (the library reads the
switch once). Every grid against the formula restated here — a workgroup per 256 items up to 8192, beyond that a quarter of that, at most
256 per CU times the switch (1 .. 1024, default 256), at least one — and with_lpp picks 1, 2, 4 for themselves and 8 for anything else.
No GPU."""
import os
import subprocess

import pytest

from aindex_amd import _lib

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(_lib.ROOT, "aindex_amd", "csrc")

WORKS = [0, 1, 256, 257, 256 * 8192, 256 * 8192 + 1, 4 * 256 * 8192, 4 * 256 * 8192 + 1024, 256 * 65536, 256 * 65536 * 4 + 1, 1 << 40]
WORKS64 = [257, 4 * 256 * 8192 + 1024, 1 << 40]                 # grid_for(work, 64)

SRC = r"""
#include <cstdio>
#include "aix_launch.hpp"

int main() {
    const unsigned long long works[] = {%s}, works64[] = {%s};
    for (unsigned long long w : works) printf("grid 256 %%llu %%u\n", w, aix::grid_for(w));
    for (unsigned long long w : works64) printf("grid 64 %%llu %%u\n", w, aix::grid_for(w, 64));
    for (unsigned lpp = 0; lpp < 10; ++lpp) printf("lpp %%u %%d\n", lpp, aix::with_lpp(lpp, [](auto L) { return (int)decltype(L)::value; }));
    return 0;
}
""" % (", ".join(f"{w}ull" for w in WORKS), ", ".join(f"{w}ull" for w in WORKS64))


def want_grid(work, per_block, per_cu):
    need = (work + per_block - 1) // per_block
    return max(min(max(min(need, 8192), need // 4), 256 * per_cu), 1)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_check")
    src = d / "launch_check.cpp"
    src.write_text(SRC)
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", f"-I{CSRC}", str(src), "-o", str(d / "launch_check")])
    return str(d / "launch_check")


@pytest.mark.parametrize("setting, per_cu", [(None, 256), ("1", 1), ("1024", 1024)])
def test_grid_and_lanes(exe, setting, per_cu):
    env = {k: v for k, v in os.environ.items() if k != "AIX_GRID_PER_CU"}
    if setting is not None:
        env["AIX_GRID_PER_CU"] = setting
    r = subprocess.run([exe], stdout=subprocess.PIPE, env=env, timeout=60)
    assert r.returncode == 0
    rows = [line.split() for line in r.stdout.decode().strip().split("\n")]
    grids = [(int(pb), int(w), int(g)) for kind, pb, w, g in (x for x in rows if x[0] == "grid")]
    assert [(pb, w) for pb, w, _ in grids] == [(256, w) for w in WORKS] + [(64, w) for w in WORKS64]
    for pb, w, g in grids:
        assert g == want_grid(w, pb, per_cu), (pb, w, g)
    assert [(int(x[1]), int(x[2])) for x in rows if x[0] == "lpp"] == [(lpp, lpp if lpp in (1, 2, 4) else 8) for lpp in range(10)]
