"""What shm_grid_field_at_points rests on that needs no GPU: the drop rule of csrc/shm_field_cull.h (tests/native/test_field_cull.cpp, stand-alone, plain and
under AddressSanitizer + UBSan) and the numpy restatement tests/field_points_ref.py, held to the fixture's Y at every node of bunny_small_n16."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import field_points_ref as ref

PLAIN = ["-O2"]
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("flags", [PLAIN, SAN], ids=["plain", "sanitizers"])
def test_field_cull_native(tmp_path, flags):
    """The bound B_c against the brute-force sum in long double, d_lo = 0 never dropped, the running sum within its limit, the acceptance test implying
    2 R / |X_kept| <= budget, and accepted scenes within budget of the full sum (the program's head lists what it holds)."""
    exe = str(tmp_path / "test_field_cull")
    src = os.path.join(ROOT, "tests", "native", "test_field_cull.cpp")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-3000:]


@pytest.fixture(scope="module")
def bunny():
    g = load_golden("bunny_small_n16")
    return dict(pos=g["pos"], wnormal=g["wnormal"], area=g["area"], lam=float(g["lam"]), n=int(g["n"]), bbox_min=g["bbox_min"], cell=float(g["cell"]), Y=g["Y"])


def test_restatement_matches_the_fixture_at_every_node(bunny):
    """At all 4096 node positions (i * cell + bbox_min) the plain restatement matches the fixture's Y within price, and the fsum form lies within the plain
    form's price (and is the cheaper of the two)."""
    pts = ref.node_positions(bunny)
    y = ref.yardstick(bunny["pos"], bunny["wnormal"], bunny["lam"], pts)
    assert y["finite"].all() and (y["lam_rmin"] < ref.ZONE).all()
    err = np.abs(y["Y"] - bunny["Y"]).max(axis=1)
    print("restatement against the fixture: max err / price = %.3f, max price %.2e, min ratio %.3f" % ((err / y["price"]).max(), y["price"].max(), y["ratio"].min()))
    assert (err <= y["price"]).all()
    ye = ref.yardstick(bunny["pos"], bunny["wnormal"], bunny["lam"], pts, exact=True)
    assert (np.abs(ye["Y"] - y["Y"]).max(axis=1) <= y["price"]).all() and (ye["price"] < y["price"]).all()
    assert (np.abs(ye["Y"] - bunny["Y"]).max(axis=1) <= y["price"]).all()


def test_families_are_finite_and_in_zone(bunny):
    """The three seeded families the GPU tests use leave no point out: every one is finite and in zone, so the excluded share there is 0."""
    for fam in ref.FAMILIES:
        pts = ref.family(fam, bunny, 2000, seed=11)
        y = ref.yardstick(bunny["pos"], bunny["wnormal"], bunny["lam"], pts)
        print("%-5s max price %.2e  min ratio %.3f  max lambda r_min %.1f" % (fam, y["price"].max(), y["ratio"].min(), y["lam_rmin"].max()))
        assert y["finite"].all() and (y["lam_rmin"] < ref.ZONE).all()
        assert y["price"].max() < 1e-10
