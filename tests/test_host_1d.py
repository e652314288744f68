"""1D on the host (no GPU): the segment mesh, the Sod and Sedov initial states, the refusals, and the driver's PA -> FA
switch (reference laghos.cpp:428-462, :499-515, :597-616, :1094-1275; data/segment01.mesh)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")


def disc(rs, ok, ot, problem, E0=1.0, nranks=1):
    from laghos_amd import host_lib
    return host_lib.host_disc("segment01", rs, ok, ot, problem, blast_energy=E0, nranks=nranks)


@pytest.mark.parametrize("rs,ok,ot", [(0, 1, 0), (1, 2, 1), (3, 3, 2), (2, 5, 4)])
def test_segment01_discretization(rs, ok, ot):
    from laghos_amd import host_lib
    d = disc(rs, ok, ot, 2)
    NE, D = 2 * 2 ** rs, ok + 1
    N = NE * ok + 1
    h1 = d["h1map"].reshape(NE, D)
    # element e holds nodes e*ok .. e*ok + ok: the nodes in natural x order, vertices shared by neighbours
    assert np.array_equal(h1, np.arange(NE)[:, None] * ok + np.arange(D)[None, :])
    assert len(d["S0"]) == 2 * N + NE * (ot + 1)
    assert list(d["ess"][0]) == [0, N - 1] and len(d["ess"][1]) == 0 and len(d["ess"][2]) == 0
    tab = host_lib.host_tables(ok, ot)
    assert np.array_equal(d["W"], tab["qwts"])
    assert len(d["nbr_rank"]) == 0 and np.all(d["owner"] == 1.0)


def test_sod_initial_state():
    """Problem 2 at rs 5 (README run 5): 64 zones of Q2Q1, x at the Gauss-Lobatto points, v = 0, rho0 = 1 | 0.1,
    gamma = 1.4, e = p / (rho (gamma - 1)) = 2.5 on both sides."""
    from laghos_amd import host_lib
    ok, ot = 2, 1
    d = disc(5, ok, ot, 2)
    NE, N, L = 64, 129, ot + 1
    S = d["S0"]
    gll = host_lib.host_tables(ok, ot)["gll"]
    h = 1.0 / NE
    x_ref = np.concatenate([e * h + h * gll[:-1] for e in range(NE)] + [[1.0]])
    assert np.allclose(S[:N], x_ref, rtol=0, atol=1e-15)
    assert np.all(S[N:2 * N] == 0.0)
    rho = d["rho0_l2"].reshape(NE, L)
    centres = (np.arange(NE) + 0.5) * h
    want = np.where(centres < 0.5, 1.0, 0.1)
    assert np.allclose(rho, want[:, None], rtol=1e-14, atol=0)
    assert np.all(d["gamma"] == 1.4)
    assert np.allclose(S[2 * N:], 2.5, rtol=1e-14, atol=0)
    assert np.allclose(d["rho0_q"].reshape(NE, -1), want[:, None], rtol=0, atol=0)


@pytest.mark.parametrize("rs,ok,ot,E0", [(0, 2, 1, 1.0), (3, 3, 2, 0.25), (2, 4, 3, 2.0)])
def test_sedov_1d_initial_energy(rs, ok, ot, E0):
    """Problem 1: the delta at the origin carries E0 / 2^dim = E0 / 2 (laghos.cpp:597-606), all of it in zone 0."""
    from laghos_amd import host_lib
    d = disc(rs, ok, ot, 1, E0=E0)
    NE, N, L = 2 * 2 ** rs, 2 * 2 ** rs * ok + 1, ot + 1
    e = d["S0"][2 * N:].reshape(NE, L)
    assert np.all(e[1:] == 0.0)
    assert np.all(d["S0"][N:2 * N] == 0.0) and np.allclose(d["rho0_l2"], 1.0, rtol=1e-14, atol=0)
    tab = host_lib.host_tables(ok, ot)
    h0 = d["S0"][ok] - d["S0"][0]
    integral = h0 * np.sum(tab["qwts"] * (tab["Bl"] @ e[0]))  # rho0 = 1
    assert abs(integral - E0 / 2) <= 1e-14 * E0


def test_1d_refusals(capfd):
    """Problems 0 and 3-7 are not defined in 1D, and 1D runs on one rank: both refused on the host, before any GPU call."""
    for p in (0, 3, 4, 5, 6, 7):
        with pytest.raises(RuntimeError):
            disc(2, 2, 1, p)
        assert f"problem {p} is not defined in 1D" in capfd.readouterr().err
    with pytest.raises(RuntimeError):
        disc(2, 2, 1, 2, nranks=2)
    assert "several ranks are not supported in 1D" in capfd.readouterr().err


def test_lgh_create_accepts_dim1():
    """lgh_create takes dim 1 (it used to refuse it as a bad argument); without a GPU it stops at the device check."""
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests create real 1D contexts)
    from laghos_amd import _lib
    L = _lib.load()
    NE, D, Q = 2, 3, 4
    h1 = np.array([0, 1, 2, 2, 3, 4], np.int32)
    ones = np.ones(64)
    cfg = _lib.LghConfig()
    cfg.dim, cfg.NE, cfg.D1D, cfg.Q1D, cfg.L1D, cfg.N = 1, NE, D, Q, D - 1, 5
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    cfg.h1_map = h1.ctypes.data_as(ip)
    for f in ("B_h1", "G_h1", "B_l2", "weights", "gamma"):
        setattr(cfg, f, ones.ctypes.data_as(dp))
    cfg.cfl = 0.5
    h = ctypes.c_void_p()
    assert L.lgh_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
    err = L.lgh_last_error()
    assert b"bad argument" not in err and b"HIP" in err, err
    cfg.Q1D = 5  # no 1D kernel for (D1D, Q1D) = (3, 5)
    assert L.lgh_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert b"Unknown kernel 0x135" in L.lgh_last_error()


def test_kernel_id_table():
    """The table of orders (visit_order / order_supported, lgh_common.hpp): of all (dim, D1D, Q1D) with dim 1..3, D1D 1..8,
    Q1D 1..12 and L1D = D1D - 1, lgh_create refuses exactly those off the fifteen ids - five orders in three dimensions -
    as LGH_ERR_UNSUPPORTED with 'Unknown kernel 0x<id>'.  It checks the id before it looks for a device and before cfl, so
    with cfl = 0 the fifteen fail further on: at the device check without a GPU, at the cfl argument with one."""
    from laghos_amd import _lib
    L = _lib.load()
    LGH_ERR_UNSUPPORTED = 2  # (include/laghos_hip.h)
    orders = {(2, 2), (3, 4), (4, 6), (5, 8), (6, 10)}
    h1 = np.zeros(4096, np.int32)
    ones = np.ones(4096)
    cfg = _lib.LghConfig()
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    cfg.h1_map = h1.ctypes.data_as(ip)
    for f in ("B_h1", "G_h1", "B_l2", "weights", "gamma"):
        setattr(cfg, f, ones.ctypes.data_as(dp))
    cfg.NE, cfg.N, cfg.cfl = 1, 1, 0.0
    h = ctypes.c_void_p()
    known = 0
    for dim in (1, 2, 3):
        for D in range(1, 9):
            for Q in range(1, 13):
                cfg.dim, cfg.D1D, cfg.Q1D, cfg.L1D = dim, D, Q, D - 1
                kid = (dim << 8) | (D << 4) | Q
                rc = L.lgh_create(ctypes.byref(cfg), ctypes.byref(h))
                err = L.lgh_last_error()
                assert rc != 0, hex(kid)
                if (D, Q) in orders:
                    known += 1
                    assert rc != LGH_ERR_UNSUPPORTED and b"Unknown kernel" not in err, (hex(kid), rc, err)
                else:
                    assert rc == LGH_ERR_UNSUPPORTED and err == b"Unknown kernel 0x%x" % kid, (hex(kid), rc, err)
    assert known == 15
    # sizes that do not fit their four bits would alias one of the fifteen ids: refused as well, by the id they pack to
    for dim, D, Q, kid in ((1, 18, 2, 0x122), (2, 18, 2, 0x322), (2, 2, 34, 0x222), (3, 3, 20, 0x334)):
        assert ((dim << 8) | (D << 4) | Q) == kid
        cfg.dim, cfg.D1D, cfg.Q1D, cfg.L1D = dim, D, Q, D - 1
        rc = L.lgh_create(ctypes.byref(cfg), ctypes.byref(h))
        err = L.lgh_last_error()
        assert rc == LGH_ERR_UNSUPPORTED and err == b"Unknown kernel 0x%x" % kid, (dim, D, Q, rc, err)


def test_driver_switches_pa_to_fa_in_1d():
    """-pa (the default) in 1D prints the reference's switch message; -fa stays refused in 2D with the same words."""
    p = subprocess.run([EXE, "-p", "2", "-m", "data/segment01.mesh", "-rs", "1", "-ms", "1", "-pa"], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert p.stdout.count("Laghos does not support PA in 1D. Switching to FA.") == 1, p.stdout + p.stderr
    p = subprocess.run([EXE, "-p", "1", "-m", "data/square01_quad.mesh", "-rs", "1", "-ms", "1", "-fa"], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert p.returncode != 0 and "laghos: only the partial-assembly path (-pa) is implemented" in p.stderr
    p = subprocess.run([EXE, "-p", "2", "-m", "data/segment01.mesh", "-rs", "1", "-ms", "1", "-fa"], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert "only the partial-assembly path" not in p.stderr and "Switching to FA" not in p.stdout
    p = subprocess.run([EXE, "-p", "3", "-dim", "1", "-nx", "8", "-ms", "1"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode != 0 and "problem 3 is not defined in 1D" in p.stderr


@pytest.mark.parametrize("problem", [1, 2])
@pytest.mark.parametrize("rs,ok,ot", [(0, 1, 0), (1, 2, 1), (3, 3, 2), (2, 4, 3), (5, 5, 4)])
def test_segment01_discretization_vs_oracle(problem, rs, ok, ot):
    """The host's 1D discretisation against the oracle's Problem (oracle/fem.py, written independently from the
    reference): initial state, rho0 (Bernstein dofs and at the quadrature points), gamma, numbering, essential dofs."""
    from oracle.fem import Problem
    d = disc(rs, ok, ot, problem)
    p = Problem(mesh="segment01", rs=rs, order_v=ok, order_e=ot, problem=problem)
    S, rho_l2, gamma, rho0_q = p.initial_state()
    assert p.dim == 1 and p.NE == 2 * 2 ** rs and p.N == p.NE * ok + 1
    assert np.array_equal(d["h1map"].reshape(p.NE, p.ND), p.h1map)
    assert np.array_equal(d["ess"][0], p.ess[0]) and len(p.ess) == 1
    assert d["S0"].shape == S.shape
    assert np.max(np.abs(d["S0"] - S)) <= 1e-14 * np.max(np.abs(S))
    assert np.max(np.abs(d["rho0_l2"] - rho_l2)) <= 1e-14
    assert np.array_equal(d["rho0_q"], rho0_q)
    assert np.array_equal(d["gamma"], gamma)
    assert np.max(np.abs(d["W"] - p.W)) <= 1e-15


@pytest.mark.parametrize("nx", [3, 7, 257])
def test_cartesian_breaks_vs_segment01(nx):
    """The oracle's `-dim 1 -nx n` mesh (breaks = linspace(0, 1, n + 1)) is segment01 refined when n = 2^(rs+1), and a
    valid 1D problem of any size otherwise: numbering, ends, node coordinates."""
    from oracle.fem import Problem
    ok = 2
    p = Problem(breaks=[np.linspace(0.0, 1.0, nx + 1)], order_v=ok, order_e=1, problem=2)
    assert p.NE == nx and p.N == nx * ok + 1
    assert np.array_equal(p.h1map, np.arange(nx)[:, None] * ok + np.arange(ok + 1)[None, :])
    assert list(p.ess[0]) == [0, p.N - 1]
    x = p.initial_state()[0][:p.N]
    assert np.all(np.diff(x) > 0) and x[0] == 0.0 and x[-1] == 1.0
    if nx == 257:
        return
    q = Problem(mesh="segment01", rs=3, order_v=ok, order_e=1, problem=2)
    r = Problem(breaks=[np.linspace(0.0, 1.0, 17)], order_v=ok, order_e=1, problem=2)
    assert np.max(np.abs(q.initial_state()[0] - r.initial_state()[0])) <= 1e-15
