"""Python mirror of LagrangianHydroOperator + RK4 + the adaptive time loop over
the C ABI (reference: /root/reference/laghos_solver.cpp:104-540, laghos.cpp:706-778).

All numerics run in liblaghos_hip.so on the GPU; this file only sequences C-ABI
calls (the same sequencing the C++ host layer in laghos_amd/host/ performs).
The problem description `prob` is duck-typed: it must provide dim, NE, D1D, Q1D,
L1D, N, H1V, L2V, h1map, B, G, Bl, W, ess, owner, order_v, use_viscosity(),
initial_state() -> (S, rho0_l2, gamma, rho0_q).
"""
import numpy as np
import torch

from .context import Context

H1, L2 = 0, 1


class HydroOperator:
    def __init__(self, prob, cfl=0.5, cg_tol=1e-8, cg_max_iter=300, device=0, comm=None):
        self.p = prob
        self.cg_tol, self.cg_max_iter = cg_tol, cg_max_iter
        S, rho_l2, gamma, rho0_q = prob.initial_state()
        multi = comm is not None and comm["nranks"] > 1
        self.ctx = ctx = Context(prob.dim, prob.NE, prob.D1D, prob.Q1D, prob.L1D, prob.N, prob.h1map,
                                 prob.B, prob.G, prob.Bl, prob.W, gamma, prob.ess,
                                 owner=prob.owner if multi else None,
                                 use_viscosity=prob.use_viscosity(),
                                 use_vorticity=getattr(prob, "use_vorticity", lambda: False)(),
                                 cfl=cfl, order_v=prob.order_v,
                                 device=device)
        self.multi = multi
        if multi:
            ctx.comm_init(comm["nranks"], comm["rank"], comm["unique_id"])
            ctx.comm_set_neighbors(comm["nbr_rank"], comm["nbr_nodes"])
        self.S0 = ctx.to_dev(S)
        x0 = ctx.clone(self.S0[:prob.H1V])
        self.rho0_l2 = ctx.to_dev(rho_l2)
        vol = ctx.setup_rho0detj0(x0, self.rho0_l2, ctx.to_dev(rho0_q))
        ne = float(prob.NE)
        if multi:
            vol = ctx.allreduce(vol, 0)
            ne = ctx.allreduce(ne, 0)
        self.volume = vol
        self.h0 = (vol / ne) ** (1.0 / prob.dim) / prob.order_v   # laghos_solver.cpp:251-262
        ctx.set_h0(self.h0)
        # scratch (laghos_solver.cpp:158-164): one, rhs, e_rhs, B
        self.one = torch.ones(prob.L2V, dtype=torch.float64, device=ctx.device)
        torch.cuda.current_stream(ctx.device).synchronize()  # torch-stream fill complete before the library reads it
        self.rhs = ctx.zeros(prob.H1V)
        self.e_rhs = ctx.zeros(prob.L2V)
        self.work = ctx.zeros(prob.N)
        # source_type 1 = 2D Taylor-Green (laghos.cpp:636-647, laghos_solver.cpp:448)
        self.e_source = ctx.zeros(prob.L2V) if (prob.problem == 0 and prob.dim == 2) else None
        # source_type 2 = gravity of problem 7 (laghos.cpp:645, laghos_solver.cpp:340-347)
        self.accel = ctx.to_dev(prob.accel_source()) if prob.problem == 7 else None
        if self.accel is not None:
            ctx.set_velocity_source(self.accel)
        self.qdata_is_current = False
        torch.cuda.synchronize()

    def close(self):
        self.ctx.close()

    # ---- `-err` post-processing (laghos.cpp:1007-1086) ----
    def compute_density(self, S):
        """LagrangianHydroOperator::ComputeDensity (laghos_solver.cpp:542-563)"""
        rho = self.ctx.zeros(self.p.L2V)
        self.ctx.compute_density(S, rho)
        return rho

    def sedov_density_error(self, S, rho, par, t, origin, weights, B_h1, G_h1, B_l2):
        """sqrt of the integrated squared density error against the exact Sedov solution `par`
        (context.sedov_setup); the error rule comes as host tables [p, d] (transposed here to the
        library's [p + n*d] layout)."""
        import numpy as np
        err2 = self.ctx.sedov_density_error(S, rho, par, t, origin, weights, np.asarray(B_h1).T.copy(),
                                            np.asarray(G_h1).T.copy(), np.asarray(B_l2).T.copy())
        return float(np.sqrt(err2))

    def diagnostics(self, S):
        """Conserved integrals, extremes and bad-point counts of the state S (Context.diagnostics): a dict by name.  Reads S
        and the set-up data only; the quadrature data stays as it is."""
        return self.ctx.diagnostics(S)

    def profile(self, S, axis, nbins, lo, hi, origin=None):
        """The state S binned along x, y, z or the distance from `origin` (Context.profile): exact, order-free bin sums and
        the curves derived from them.  Reads S and the set-up data only; the quadrature data stays as it is."""
        return self.ctx.profile(S, axis, nbins, lo, hi, origin)

    def map(self, S, cells, lo, hi):
        """The state S binned onto a fixed Cartesian grid of `cells` per axis over the box [lo, hi) (Context.map): exact,
        order-free cell sums and the fields derived from them.  Reads S and the set-up data only."""
        return self.ctx.map(S, cells, lo, hi)

    def derived_fields(self, S, R):
        """The derived fields of the state S on the lattice of R cells per zone and direction (Context.sample_derived; what
        `-pv-fields` adds to a dump): a dict of numpy arrays detj, div_v, sound_speed (NP), grad_v (dim^2, NP; entry i*dim + j =
        dv_i/dx_j) and, in 2D and 3D, vorticity (NP or (3, NP)).  Reads S and the set-up data only."""
        import numpy as np
        from . import host_lib
        p, ctx = self.p, self.ctx
        dim, NP = p.dim, p.NE * (R + 1) ** p.dim
        Bh, Bl = host_lib.host_lattice_tables(p.order_v, p.order_e, R)
        Gh = host_lib.host_lattice_grad_table(p.order_v, R)
        nan = lambda n: ctx.to_dev(np.full(n, np.nan))   # (an entry the library did not write would show)
        out = dict(detj=nan(NP), grad_v=nan(dim * dim * NP), div_v=nan(NP), sound_speed=nan(NP))
        if dim > 1:
            out["vorticity"] = nan(NP if dim == 2 else 3 * NP)
        ctx.sample_derived(S, Bh, Gh, Bl, **out)
        ctx.sync()
        shape = dict(grad_v=(dim * dim, NP), vorticity=(NP,) if dim == 2 else (3, NP))
        return {k: t.cpu().numpy().reshape(shape.get(k, (NP,))) for k, t in out.items()}

    FACE_FIELDS = ("x", "v", "e", "rho", "p", "detj", "grad_v", "div_v", "vorticity", "sound_speed", "area_normal")

    def face_fields(self, S, R, faces, fields=None):
        """The fields of the state S on the lattices of R cells per direction of the zone faces `faces` ((nfaces, 2) ints: zone, local
        face 2 axis + side; Context.sample_faces; what `-pv-surface` / `-pv-slice` write): a dict of numpy arrays over NPt = nfaces
        (R+1)^(dim-1) points - x, v, area_normal (dim, NPt), e, rho, p, detj, div_v, sound_speed (NPt), grad_v (dim^2, NPt), vorticity
        (NPt or (3, NPt)) - restricted to `fields` where given, and `faces` itself.  The density is projected on the mesh of S as
        the dumps do.  Reads S and the set-up data only; 2D and 3D."""
        import numpy as np
        from . import host_lib
        p, ctx = self.p, self.ctx
        dim = p.dim
        faces = np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 2))
        fields = self.FACE_FIELDS if fields is None else tuple(fields)
        unknown = [k for k in fields if k not in self.FACE_FIELDS]
        if unknown:
            raise ValueError(f"face_fields: unknown fields {unknown}")
        NPt = faces.shape[0] * (R + 1) ** (dim - 1)
        Bh, Bl = host_lib.host_lattice_tables(p.order_v, p.order_e, R)
        Gh = host_lib.host_lattice_grad_table(p.order_v, R)
        ncomp = dict(x=dim, v=dim, grad_v=dim * dim, vorticity=3 if dim == 3 else 1, area_normal=dim)
        out = {k: ctx.to_dev(np.full(ncomp.get(k, 1) * NPt, np.nan)) for k in fields}   # (an entry the library did not write would show)
        rho = self.compute_density(S) if ("rho" in fields or "p" in fields) else None
        ctx.sample_faces(S, rho, Bh, Gh, Bl, faces, **out)
        ctx.sync()
        res = {k: (t.cpu().numpy().reshape(ncomp[k], NPt) if ncomp.get(k, 1) > 1 else t.cpu().numpy()) for k, t in out.items()}
        res["faces"] = faces
        return res

    def update_records(self, S, R, rec, t, dtr=0.0, threshold=None, first=False, faces=None):
        """One update of a block of running records (Context.records_update; the driver's `-peaks`): p, rho, e and v of the state S are
        sampled on the volume lattice of R cells per zone and direction - or, with `faces` ((nfaces, 2) ints), on those face
        lattices - as the dumps sample them, and folded into rec, a device tensor of 8 n doubles (column-major, the columns of
        Context.RECORD_COLS), at time t, dtr since the last update.  first: the update that starts the records.  Returns n.
        Asynchronous; reads S and the set-up data, writes rec only."""
        import numpy as np
        from . import host_lib
        p, ctx = self.p, self.ctx
        dim = p.dim
        if faces is not None:
            faces = np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 2))
        n = p.NE * (R + 1) ** dim if faces is None else faces.shape[0] * (R + 1) ** (dim - 1)
        Bh, Bl = host_lib.host_lattice_tables(p.order_v, p.order_e, R)
        rho_l2 = self.compute_density(S)
        f = dict(v=ctx.empty(dim * n), e=ctx.empty(n), rho=ctx.empty(n), p=ctx.empty(n))
        if faces is None:
            ctx.sample_fields(S, rho_l2, Bh, Bl, **f)
        elif n:
            ctx.sample_faces(S, rho_l2, Bh, None, Bl, faces, **f)
        ctx.records_update(dim, f["p"], f["rho"], f["e"], f["v"], t, dtr, rec, threshold=threshold, first=first)
        ctx.sync()   # (the scratch tensors go out of scope here)
        return n

    def gauges(self, zone, xi, capacity=256):
        """A set of gauges (Context.gauges_create; the driver's `-gauges`): material points given as zone[g] - this rank's zone id, -1
        where another rank owns the gauge - and reference coordinates xi (n, dim).  Returns the handle for Context.gauges_sample /
        gauges_pending / gauges_drain; the gauge's mass rho0 detJ0 comes from the initial state this operator was set up with.
        Collective on several ranks."""
        from . import host_lib
        p, ctx = self.p, self.ctx
        xi = np.asarray(xi, dtype=np.float64).reshape(-1, p.dim)
        Bh, Gh, Bl = host_lib.host_gauge_tables(p.order_v, p.order_e, xi)
        return ctx.gauges_create(zone, Bh, Gh, Bl, ctx.clone(self.S0[:p.H1V]), self.rho0_l2, capacity)

    CONTOUR_FIELDS = ("density", "energy", "pressure", "speed", "x", "y", "z", "div_v", "detj", "sound_speed")
    CONTOUR_EXTRA = ("detj", "grad_v", "div_v", "vorticity", "sound_speed")

    def contour(self, S, R, field, value=None, fields=None):
        """The contour `field` = `value` of the state S, formed on the lattice of R cells per zone and direction (Context.contour;
        what `-pv-iso` / `-pv-plane` write): `field` one of CONTOUR_FIELDS, or ("plane", normal, d) for the cut plane normal . x = d.
        Triangles in 3D, segments in 2D, points not shared: a dict with points (dim, nv), cells (nprim, dim) - indices into the
        points -, zone (nprim), v (dim, nv), e, rho, p (nv), the derived arrays named in `fields` (of CONTOUR_EXTRA) interpolated the
        same way, n_skipped, and the contour itself (edges (nprim, dim, 2), t (nprim, dim): Context.contour).  The density is projected on the mesh of S as the dumps do.  Reads S and the set-up data only."""
        import numpy as np
        from . import host_lib
        p, ctx = self.p, self.ctx
        dim, R1 = p.dim, R + 1
        if dim == 1:
            raise ValueError("contour: 2D and 3D")
        plane = None
        if not isinstance(field, str):
            kind, normal, d = field
            plane = np.asarray(normal, dtype=np.float64).reshape(-1)
            if kind != "plane" or plane.size != dim or not np.all(np.isfinite(plane)) or not np.any(plane != 0):
                raise ValueError(f"contour: {field!r} is no plane of a {dim}D mesh")
            value = d
        elif field not in self.CONTOUR_FIELDS or (field == "z" and dim == 2):
            raise ValueError(f"contour: unknown field {field!r}")
        if value is None or not np.isfinite(value):
            raise ValueError(f"contour: the value {value!r} is not a finite number")
        extra = tuple(fields or ())
        unknown = [k for k in extra if k not in self.CONTOUR_EXTRA]
        if unknown:
            raise ValueError(f"contour: unknown fields {unknown}")
        NP = p.NE * R1 ** dim
        Bh, Bl = host_lib.host_lattice_tables(p.order_v, p.order_e, R)
        lat = dict(x=ctx.empty(dim * NP), v=ctx.empty(dim * NP), e=ctx.empty(NP), rho=ctx.empty(NP), p=ctx.empty(NP))
        ctx.sample_fields(S, self.compute_density(S), Bh, Bl, **lat)
        ncomp = dict(x=dim, v=dim, grad_v=dim * dim, vorticity=3 if dim == 3 else 1)
        need = set(extra) | ({field} if field in self.CONTOUR_EXTRA else set())
        if need:
            der = {k: ctx.empty(ncomp.get(k, 1) * NP) for k in self.CONTOUR_EXTRA if k in need}
            ctx.sample_derived(S, Bh, host_lib.host_lattice_grad_table(p.order_v, R), Bl, **der)
            lat.update(der)
        if plane is not None:
            scalar = ctx.contour_scalar("plane", lat["x"], plane)
        elif field in ("x", "y", "z"):
            scalar = ctx.contour_scalar("plane", lat["x"], np.eye(3)["xyz".index(field)][:dim])
        elif field == "speed":
            scalar = ctx.contour_scalar("norm", lat["v"])
        else:
            scalar = lat[dict(density="rho", energy="e", pressure="p").get(field, field)]
        edges, t, zone, n_skipped = ctx.contour(scalar, value, R1)
        out = {k: ctx.contour_gather(edges, t, lat[k], ncomp.get(k, 1)) for k in ("x", "v", "e", "rho", "p") + extra}
        ctx.sync()
        nprim = zone.numel()
        res = {k: (a.cpu().numpy() if ncomp.get(k, 1) > 1 else a.cpu().numpy().reshape(-1)) for k, a in out.items()}
        res["points"] = res.pop("x")
        res.update(cells=np.arange(dim * nprim, dtype=np.int64).reshape(nprim, dim), zone=zone.cpu().numpy(), n_skipped=n_skipped,
                   edges=edges.cpu().numpy(), t=t.cpu().numpy())
        return res

    def loads(self, S, groups):
        """Pressure loads of the state S on groups of zone faces (Context.loads; what `-loads` writes): `groups` a list of
        (name, faces), faces (n, 2) ints (zone, local face 2 axis + side); a face may stand in several groups.  A dict with `names`,
        `rows` ((ngroups, 11) by context.LOADS_COLS), `n_excluded`, `force` (rows[:, 2:2+dim]) and `p_mean` (pa / area, NaN for an
        empty row).  The density is projected on the mesh of S as the dumps do.  Reads S and the set-up data only; 2D and 3D."""
        import numpy as np
        from .context import loads_dict
        lists = [np.asarray(f, dtype=np.int32).reshape(-1, 2) for _, f in groups]
        faces = np.concatenate([np.concatenate([f, np.full((len(f), 1), r, np.int32)], 1) for r, f in enumerate(lists)]) if lists else np.zeros((0, 3), np.int32)
        rows, n_excl = self.ctx.loads(S, self.compute_density(S), faces, len(lists))
        return loads_dict([name for name, _ in groups], rows, n_excl, self.p.dim)

    def reset_time_step_estimate(self):
        self.ctx.set_dt_est(float("inf"))

    def reset_quadrature_data(self):
        self.qdata_is_current = False
        self.ctx.reset_quadrature_data()  # the force products formed with the stale data go with it

    def update_quadrature_data(self, S):
        if self.qdata_is_current:
            return
        self.qdata_is_current = True
        self.ctx.qupdate(S)

    def get_time_step_estimate(self, S):
        self.update_quadrature_data(S)
        dt = self.ctx.get_dt_est()
        if self.multi:
            dt = self.ctx.allreduce(dt, 1)
        return dt

    def mult(self, S, dS):
        p, ctx = self.p, self.ctx
        ctx.vec_copy(dS[:p.H1V], S[p.H1V:2 * p.H1V])             # dx_dt = v
        self.update_quadrature_data(S)
        # SolveEnergy takes v from S, not from SolveVelocity: the library overlaps the two
        if self.e_source is not None:
            ctx.tg_source_2d(S, self.e_source)
        ctx.solve_energy_begin(S, S[p.H1V:2 * p.H1V], dS, self.e_rhs, self.cg_tol, self.cg_max_iter,
                               e_source=self.e_source)
        ctx.solve_velocity(S, dS, None, self.rhs, self.work, self.cg_tol, self.cg_max_iter)  # (one: the operator's own)
        ctx.solve_energy_end()
        self.qdata_is_current = False

    def e_norm(self, S):
        e = S[2 * self.p.H1V:]
        n2 = self.ctx.vec_dot(e, e)
        if self.multi:
            n2 = self.ctx.allreduce(n2, 0)
        return float(np.sqrt(n2))


def rk4_step(hydro, S, t, dt, work):
    """Classical RK4, the update sequence of upstream RK4Solver::Step."""
    ctx = hydro.ctx
    k, y, z = work
    hydro.mult(S, k)
    ctx.vec_axpby(y, 1.0, S, dt / 2, k)
    ctx.vec_axpby(z, 1.0, S, dt / 6, k)
    hydro.mult(y, k)
    ctx.vec_axpby(y, 1.0, S, dt / 2, k)
    ctx.vec_axpby(z, 1.0, z, dt / 3, k)
    hydro.mult(y, k)
    ctx.vec_axpby(y, 1.0, S, dt, k)
    ctx.vec_axpby(z, 1.0, z, dt / 3, k)
    hydro.mult(y, k)
    ctx.vec_axpby(S, 1.0, z, dt / 6, k)
    return t + dt


def rk1_step(hydro, S, t, dt, work):
    """upstream ForwardEulerSolver::Step"""
    k = work[0]
    hydro.mult(S, k)
    hydro.ctx.vec_axpby(S, 1.0, S, dt, k)
    return t + dt


def rk2_step(hydro, S, t, dt, work, a=0.5):
    """upstream RK2Solver(a)::Step; Laghos uses a = 0.5, the midpoint rule (laghos.cpp:522)"""
    ctx = hydro.ctx
    k, x1, _ = work
    b = 0.5 / a
    hydro.mult(S, k)
    ctx.vec_axpby(x1, 1.0, S, (1.0 - b) * dt, k)
    ctx.vec_axpby(S, 1.0, S, a * dt, k)
    hydro.mult(S, k)
    ctx.vec_axpby(S, 1.0, x1, b * dt, k)
    return t + dt


def rk3ssp_step(hydro, S, t, dt, work):
    """upstream RK3SSPSolver::Step (laghos.cpp:523)"""
    ctx = hydro.ctx
    k, y, _ = work
    hydro.mult(S, k)
    ctx.vec_axpby(y, 1.0, S, dt, k)
    hydro.mult(y, k)
    ctx.vec_axpby(y, 1.0, y, dt, k)
    ctx.vec_axpby(y, 3.0 / 4, S, 1.0 / 4, y)
    hydro.mult(y, k)
    ctx.vec_axpby(y, 1.0, y, dt, k)
    ctx.vec_axpby(S, 1.0 / 3, S, 2.0 / 3, y)
    return t + dt



# upstream RK6Solver (laghos.cpp:525): Verner's 8-stage 6th-order method, upstream's coefficients; the
# order conditions through order 6 hold to 1e-30 (tests/test_host_setup.py)
RK6_A = [
    .6e-1,
    .1923996296296296296296296296296296296296e-1, .7669337037037037037037037037037037037037e-1,
    .35975e-1, 0., .107925,
    1.318683415233148260919747276431735612861, 0., -5.042058063628562225427761634715637693344,
    4.220674648395413964508014358284402080483,
    -41.87259166432751461803757780644346812905, 0., 159.4325621631374917700365669070346830453,
    -122.1192135650100309202516203389242140663, 5.531743066200053768252631238332999150076,
    -54.43015693531650433250642051294142461271, 0., 207.0672513650184644273657173866509835987,
    -158.6108137845899991828742424365058599469, 6.991816585950242321992597280791793907096,
    -.1859723106220323397765171799549294623692e-1,
    -54.66374178728197680241215648050386959351, 0., 207.9528062553893734515824816699834244238,
    -159.2889574744995071508959805871426654216, 7.018743740796944434698170760964252490817,
    -.1833878590504572306472782005141738268361e-1, -.5119484997882099077875432497245168395840e-3]
RK6_B = [
    .3438957868357036009278820124728322386520e-1, 0., 0., .2582624555633503404659558098586120858767,
    .4209371189673537150642551514069801967032, 4.405396469669310170148836816197095664891,
    -176.4831190242986576151740942499002125029, 172.3641334014150730294022582711902413315]


def rk6_step(hydro, S, t, dt, work):
    """upstream ExplicitRKSolver::Step with the RK6Solver tableau (same order of operations)"""
    ctx = hydro.ctx
    if getattr(hydro, "_rk6_k", None) is None or hydro._rk6_k[0].numel() != S.numel():
        hydro._rk6_k = [torch.empty_like(S) for _ in range(8)]
        torch.cuda.synchronize()
    k, y = hydro._rk6_k, work[1]
    hydro.mult(S, k[0])
    l = 0
    for i in range(1, 8):
        ctx.vec_axpby(y, 1.0, S, RK6_A[l] * dt, k[0])
        l += 1
        for j in range(1, i):
            ctx.vec_axpby(y, 1.0, y, RK6_A[l] * dt, k[j])
            l += 1
        hydro.mult(y, k[i])
    for i in range(8):
        ctx.vec_axpby(S, 1.0, S, RK6_B[i] * dt, k[i])
    return t + dt


def rk2avg_step(hydro, S, t, dt, work):
    """RK2AvgSolver::Step (laghos_solver.cpp:1447-1487): two SolveVelocity /
    SolveEnergy sub-steps, the energy one with the half-step average velocity V."""
    ctx, p = hydro.ctx, hydro.p
    dS, S0, y = work
    h1v = p.H1V
    V = y[:h1v]
    ctx.vec_copy(S0, S)
    v0, dv = S0[h1v:2 * h1v], dS[h1v:2 * h1v]
    for sub in (0, 1):
        if sub == 1:
            ctx.vec_axpby(S, 1.0, S0, 0.5 * dt, dS)                # S = S0 + dt/2 dS_dt
            hydro.reset_quadrature_data()
        hydro.update_quadrature_data(S)
        ctx.solve_velocity(S, dS, None, hydro.rhs, hydro.work, hydro.cg_tol, hydro.cg_max_iter)
        ctx.vec_axpby(V, 1.0, v0, 0.5 * dt, dv)                   # V = v0 + dt/2 dv_dt
        if hydro.e_source is not None:
            ctx.tg_source_2d(S, hydro.e_source)
        ctx.solve_energy(S, V, dS, hydro.e_rhs, hydro.cg_tol, hydro.cg_max_iter, e_source=hydro.e_source)
        ctx.vec_copy(dS[:h1v], V)                                  # dx_dt = V
    ctx.vec_axpby(S, 1.0, S0, dt, dS)                              # S = S0 + dt dS_dt
    hydro.reset_quadrature_data()
    return t + dt


class TimeLoop:
    """laghos.cpp:706-778 as a resumable object (bench.py steps it K times)."""

    def __init__(self, hydro, t_final=0.6, max_steps=-1, ode_solver=4):
        steppers = {1: rk1_step, 2: rk2_step, 3: rk3ssp_step, 4: rk4_step, 6: rk6_step, 7: rk2avg_step}
        if ode_solver not in steppers:
            raise ValueError("ode_solver: 1 (Euler), 2 (RK2), 3 (RK3 SSP), 4 (RK4), 6 (RK6) or 7 (RK2Avg)")
        self.stepper = steppers[ode_solver]
        self.h = hydro
        self.t_final, self.max_steps = t_final, max_steps
        self.S = hydro.S0.clone()
        self.S_old = self.S.clone()
        self.work = tuple(torch.empty_like(self.S) for _ in range(3))
        torch.cuda.synchronize()  # torch-stream clones visible to the context stream
        hydro.reset_time_step_estimate()
        self.t = 0.0
        self.dt = hydro.get_time_step_estimate(self.S)
        self.ti = 1
        self.steps = 0
        self.repeats = 0
        self.last_step = False

    def step(self):
        """Advance one accepted time step (repeating with smaller dt as needed).
        Returns False when the run is finished."""
        h = self.h
        while True:
            if self.last_step:
                return False
            if self.t + self.dt >= self.t_final:
                self.dt = self.t_final - self.t
                self.last_step = True
            if self.steps == self.max_steps:
                self.last_step = True
            h.ctx.vec_copy(self.S_old, self.S)
            t_old = self.t
            h.reset_time_step_estimate()
            self.t = self.stepper(h, self.S, self.t, self.dt, self.work)
            self.steps += 1
            dt_est = h.get_time_step_estimate(self.S)
            if dt_est < self.dt:
                self.dt *= 0.85
                if self.dt < np.finfo(float).eps:
                    raise RuntimeError("The time step crashed!")
                self.t = t_old
                h.ctx.vec_copy(self.S, self.S_old)
                h.reset_quadrature_data()
                self.repeats += 1
                if self.steps < self.max_steps:
                    self.last_step = False
                continue
            elif dt_est > 1.25 * self.dt:
                self.dt *= 1.02
            self.ti += 1
            return True


def run(prob, t_final=0.6, cfl=0.5, cg_tol=1e-8, cg_max_iter=300, max_steps=-1, probe_steps=(),
        device=0, comm=None, ode_solver=4, timers=True):
    hydro = HydroOperator(prob, cfl=cfl, cg_tol=cg_tol, cg_max_iter=cg_max_iter, device=device, comm=comm)
    hydro.ctx.enable_timers(timers)  # off: the energy solve overlaps the velocity solve (lgh_solve_energy_begin)
    loop = TimeLoop(hydro, t_final=t_final, max_steps=max_steps, ode_solver=ode_solver)
    probes = {}
    while loop.step():
        done_ti = loop.ti - 1
        if done_ti in probe_steps:
            probes[done_ti] = hydro.e_norm(loop.S)
    out = dict(probes=probes, steps=loop.steps, repeats=loop.repeats, ti=loop.ti - 1, t=loop.t,
               dt=loop.dt, e_norm=hydro.e_norm(loop.S), S=loop.S.cpu().numpy(), timers=hydro.ctx.timers())
    hydro.close()
    return out
