"""Pins the CPU oracle against the reference's own golden vectors:
the `--checks` table (laghos.cpp:1441-1463) and the README / `make tests` runs
(README.md:225-235, makefile:271-278).  No GPU, no product code."""
import json
import os

import pytest

from oracle.driver import run
from oracle.fem import Problem

CHECK_NAMES = ["chk-3D-Sedov", "chk-2D-Sedov", "chk-3D-TG", "chk-2D-TG", "chk-3D-p3", "chk-2D-p3"] + \
              [f"chk-{d}D-p{p}" for p in (2, 4, 5, 6, 7) for d in (3, 2)]  # = `make checks`: problems 0-7 x {2D, 3D}


@pytest.mark.parametrize("name", CHECK_NAMES)
def test_checks_table(golden, name):
    g = next(c for c in golden["checks"] if c["name"] == name)
    probes = {int(k): v for k, v in g["probes"].items()}
    # options asserted by the reference for --checks: laghos.cpp:909-917, makefile:199
    r = run(Problem(mesh=g["mesh"], rs=0, order_v=2, order_e=1, problem=g["problem"]),
            t_final=0.6, cfl=0.5, cg_tol=1e-14, probe_steps=tuple(probes))
    for step, ref in probes.items():
        got = r["probes"][step]
        # reference bar: rel 1e-13 (laghos.cpp:1419-1429); the oracle is held to 1e-12
        assert abs(got - ref) / ref < 1e-12, (name, step, got, ref)


README_NAMES = ["README-1", "README-2", "README-3", "README-4", "README-6", "README-7", "README-8", "README-9"]


@pytest.mark.parametrize("name", README_NAMES)
def test_readme_runs(golden, name):
    g = next(c for c in golden["readme"] if c["name"] == name)
    r = run(Problem(mesh=g["mesh"], rs=g["rs"], problem=g["problem"], blast_energy=g["E0"],
                    order_v=g.get("order_v", 2), order_e=g.get("order_e", 1)),
            t_final=g["tf"], ode_solver=g.get("ode_solver", 4))  # default -cgt 1e-8, -cfl 0.5, Q2Q1, RK4
    last = r["last"]
    assert last["step"] == g["step"]
    assert f"{last['dt']:.6f}" == g["dt"]
    # the README prints 11 significant digits: "within round-off distance" (README.md:249-250)
    if "e_rel_tol" in g:  # run 9: see the fixture's comment
        assert abs(last["e_norm"] - g["e_norm"]) / g["e_norm"] < g["e_rel_tol"], (last["e_norm"], g["e_norm"])
    else:
        assert f"{last['e_norm']:.10e}" == f"{g['e_norm']:.10e}", (last["e_norm"], g["e_norm"])


def test_readme_run5_fa_branch():
    """README run 5 (1D Sod, Q2Q1, RK4, 64 zones) through the oracle's full-assembly branch, against the published row
    (tests/golden/readme_run5.json).  The row was printed by 8 MPI ranks (README.md:219); the oracle runs the serial
    sums, and still reproduces all 11 published digits of |e|, so the digits are asserted as for the other runs."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readme_run5.json")) as f:
        g = json.load(f)
    r = run(Problem(mesh="segment01", rs=5, problem=2, order_v=2, order_e=1), t_final=0.2)
    last = r["last"]
    assert last["step"] == g["step"] == 413
    assert f"{last['dt']:.6f}" == g["dt"] == "0.000470"
    assert f"{last['e_norm']:.10e}" == f"{g['e_norm']:.10e}" == "3.2012077410e+01", last["e_norm"]
    # the run repeats steps (dt control, laghos.cpp:748-760): the 1D oracle exercises that path too
    assert r["repeats"] > 0
