"""The extended-precision yardstick (tests/highprec_ref.py) against mpmath alone, and the CPU oracle against the yardstick
entry by entry on every case that tests/test_highprec_gpu.py runs on the device.  The second part measures K_oracle, the
oracle's largest distance d = |oracle - yardstick| / (2^-53 S) per (module, input family), prints it, and fails when it
exceeds the constant recorded in highprec_ref.K_ORACLE (from which the device's bound is taken)."""
import mpmath
import numpy as np
import pytest

import highprec_ref as H

LD = np.longdouble


# ---- the yardstick against mpmath alone ----------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [2, 4, 6, 8])
def test_quadrature_is_exact_for_monomials_up_to_its_degree(degree):
    n = H.gauss_npts(degree)
    xs, ws = H.gauss_mp(n)
    with mpmath.workdps(40):
        for k in range(2 * n):                                   # n points: exact to degree 2n - 1 >= degree
            exact = mpmath.mpf(2) / (k + 1) if k % 2 == 0 else mpmath.mpf(0)
            assert abs(sum(w * x ** k for x, w in zip(xs, ws)) - exact) < mpmath.mpf(10) ** -35, k
        assert abs(sum(w * x ** (2 * n) for x, w in zip(xs, ws)) - mpmath.mpf(2) / (2 * n + 1)) > mpmath.mpf(10) ** -6
    assert 2 * n - 1 >= degree
    x, w, _, _ = H.line_tables(1, n)                             # the rounded tables
    for k in range(2 * n):
        assert abs(float((w * x ** k).sum()) - (2.0 / (k + 1) if k % 2 == 0 else 0.0)) < 4e-19


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_lagrange_partition_of_unity_and_kronecker(order):
    _, _, V, D = H.line_tables(order, order + 1)
    assert np.abs(V.sum(axis=0) - 1).max() < 4e-19 * (order + 1) and np.abs(D.sum(axis=0)).max() < 1e-17
    N = H.node_tables(order, order)
    assert np.array_equal(N, np.eye(order + 1, dtype=LD))
    with mpmath.workdps(40):                                     # the derivative against mpmath's own differentiation
        x0 = mpmath.mpf("0.3137")
        _, der = H.lagrange_mp(order, x0)
        for k in range(order + 1):
            assert abs(der[k] - mpmath.diff(lambda x: H.lagrange_mp(order, x)[0][k], x0)) < mpmath.mpf(10) ** -25


def _sheared_hex():
    v = np.array([[a, b, c] for c in (0, 1) for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))], dtype=np.float64)
    A = np.array([[1.25, 0.5, -0.25], [-0.5, 0.75, 0.375], [0.125, -0.25, 1.5]])      # exact in binary
    return v @ A.T + 0.5, A


@pytest.mark.parametrize("order", [1, 2])
def test_thermal_stiffness_sums_to_zero_and_mass_sums_to_the_volume(order):
    nodes, A = _sheared_hex()
    n = (order + 1) ** 3
    m = dict(nodes=nodes[None], lids=np.arange(n)[None], offsets=np.arange(n), ndof=n)
    blk = H.Block(m, 2 * order, order=order)
    u = np.random.default_rng(3).uniform(-1, 1, n)
    P = dict(source=0.0, diffusion=1.7, rho=1.0, cp=1.0, adv=None)
    el = H.element_arrays(blk, "thermal", P, u)
    assert abs(float(el["local_J"].sum())) < 4e-19 * float(el["S_J"].sum())
    assert np.abs(el["local_J"].sum(axis=2)).max() < 4e-19 * float(el["S_J"].sum(axis=2).max())   # constants: no flux
    with mpmath.workdps(40):
        vol = mpmath.det(mpmath.matrix(A.tolist()))              # the sheared unit cube
    tr = dict(H.TABLEAU, stage=0, butcher_A=np.array([[1.0]]), butcher_b=np.array([1.0]), bdf=np.array([1.0, -1.0]), dt=1.0,
              u_prev=np.zeros((n, 1)), u_stage=np.zeros((n, 1)))
    mass = H.element_arrays(blk, "thermal", dict(P, diffusion=0.0), u, tr)["local_J"]          # alpha_t = 1: the mass matrix
    assert abs(mass.sum() - H._ld(vol)) < 8e-19 * float(vol)


@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("dim", [2, 3])
def test_complex_step_matches_mpmath_diff_of_the_navierstokes_point_function(dim, rest):
    """C = dF/dU of the navierstokes point function, SUPG + PSPG, transient, by the complex step in clongdouble against
    mpmath.diff of the same expressions written on mpf (the point function is plain arithmetic: it runs on mpf as it
    stands, with sqrt and where taken from mpmath), at a state with |u| = O(1) and at rest."""
    S, K = 1 + dim, (dim + 1) * (1 + dim)
    rng = np.random.default_rng(5)
    U0 = rng.uniform(-1, 1, K)
    if rest:
        U0[[0, 2 * S] + ([3 * S] if dim == 3 else [])] = 0.0
    Ud0 = rng.uniform(-1, 1, K)
    x = np.full((1, 1, dim), 0.25, LD)
    P = {"source ux": 0.3, "source uy": 0.7, "source uz": -0.2, "viscosity": 0.05, "density": 1.3, "useSUPG": 1,
         "usePSPG": 1, "h": np.full((1, 1), LD(0.37)), "dt": 0.05, "transient": True}
    U, Ud = U0.astype(LD).reshape(K, 1, 1), Ud0.astype(LD).reshape(K, 1, 1)
    F, CU, CT = H.point_derivative(H.navierstokes_point, U, Ud, x, P)

    def F_mp(Uv, Udv):                                          # the same formulas (navierstokes.cpp) on mpf
        dens, visc, h, dt = mpmath.mpf(1.3), mpmath.mpf(0.05), mpmath.mpf(float(LD(0.37))), mpmath.mpf(0.05)
        src = [mpmath.mpf(0.3), mpmath.mpf(0.7), mpmath.mpf(-0.2)][:dim]
        vn = [0, 2, 3][:dim]
        vel = [Uv[v * S] for v in vn]
        nvel = sum(v * v for v in vel)
        if nvel > mpmath.mpf("1e-12"):
            nvel = mpmath.sqrt(nvel)
        tau = 1 / mpmath.sqrt((4 * visc / h / h) ** 2 + (2 * nvel / h) ** 2 + (2 / dt) ** 2)
        out = [None] * K
        divu = 0
        for i, v in enumerate(vn):
            b = v * S
            conv = sum(vel[d] * Uv[b + 1 + d] for d in range(dim))
            out[b] = dens * (Udv[b] + conv - src[i])
            strong = dens * Udv[b] + dens * conv + Uv[S + 1 + i] - dens * src[i]
            for d in range(dim):
                out[b + 1 + d] = visc * Uv[b + 1 + d] - (Uv[S] if d == i else 0) + tau * strong * vel[d]
            out[S + 1 + i] = strong * tau / dens
            divu += Uv[b + 1 + i]
        out[S] = divu
        return out

    with mpmath.workdps(40):
        Um, Udm = [mpmath.mpf(float(v)) for v in U0], [mpmath.mpf(float(v)) for v in Ud0]
        Fm = F_mp(Um, Udm)
        scale = max(abs(f) for f in Fm)
        for k in range(K):
            assert abs(H._ld(Fm[k]) - F[k, 0, 0]) < 1e-18 * float(scale), k
            for l in range(K):
                def f(t, k=k, l=l):
                    return F_mp([u + (t if j == l else 0) for j, u in enumerate(Um)], Udm)[k]
                ref = mpmath.diff(f, 0) if not (rest and l % S == 0 and l != S) else mpmath.diff(f, 0, h=mpmath.mpf("1e-25"))
                assert abs(H._ld(ref) - CU[k, l, 0, 0]) < 1e-17 * max(1.0, float(abs(ref))), (k, l, float(ref), float(CU[k, l, 0, 0]))
            for l in range(0, K, S):
                def g(t, k=k, l=l):
                    return F_mp(Um, [u + (t if j == l else 0) for j, u in enumerate(Udm)])[k]
                assert abs(H._ld(mpmath.diff(g, 0)) - CT[k, l, 0, 0]) < 1e-17 * max(1.0, float(abs(mpmath.diff(g, 0)))), (k, l)


def _fields_of_c(module):
    """cdr's deck strings that read the fields, as callables on the slot values (highprec_ref.later_case_data)."""
    return {"reaction": (lambda f: 0.5 * f["c"] * f["c"] + 0.1 * f["grad(c)[x]"] * f["grad(c)[x]"], "0.5*c*c + 0.1*grad(c)[x]^2"),
            "diffusion": (lambda f: (1 + 0.1 * f["x"]) + f["c"] * f["c"], "kappa0+c*c"),
            "xvel": (lambda f: f["ux"], "ux") if module == "navierstokes+cdr" else (lambda f: f["c"], "c"),
            "yvel": (lambda f: 0.3 * f["c_t"], "0.3*c_t")}


NS_NUMBERS = {"source ux": 0.3, "source uy": 0.7, "source uz": -0.2, "viscosity": 0.05, "density": 1.3, "useSUPG": 1, "usePSPG": 1,
              "dt": 0.05, "transient": True}
POINT_PARAMS = {     # numbers only (they go to mpf as they stand); every switch on
    "stokes": {"source ux": 0.3, "source uy": 0.7, "source uz": -0.2, "viscosity": 0.7, "usePSPG": 1, "useLSIC": 1},
    "shallowwater": {"bathymetry": 1.1, "bathymetry_x": 0.3, "bathymetry_y": -0.2, "source H": 0.2, "source Hu": 0.4, "source Hv": -0.1},
    "helmholtz": {"c2r_x": 1.3, "c2r_y": 0.8, "c2r_z": 1.9, "c2i_x": 0.4, "c2i_y": -0.6, "c2i_z": 0.25, "omega2r": 2.1,
                  "omega2i": 0.3, "source_r": 2.0, "source_i": -1.5},
    "cdr": {"source": 2.0, "specific heat": 1.4, "density": 1.3, "zvel": 0.4},
    "navierstokes+cdr": dict(NS_NUMBERS, **{"source": 2.0, "specific heat": 1.4, "zvel": 0.4}),
    "navierstokes+thermal": dict(NS_NUMBERS, **{"thermal source": 3.0, "thermal diffusion": 1.7, "specific heat": 1.4, "beta": 0.7,
                                                "T_ambient": 0.3, "include advection": 1, "bx": 0.8, "by": -0.5, "bz": 0.3}),
    "linearelasticity+thermal": {"lambda": 1.1, "mu": 0.6, "source dx": 0.3, "source dy": 0.7, "source dz": -0.2, "thermal source": 3.0,
                                 "thermal diffusion": 1.7, "specific heat": 1.4, "density": 1.3, "incplanestress": 1, "alpha_T": 0.35,
                                 "T_ambient": 0.3, "include advection": 1, "bx": 0.8, "by": -0.5, "bz": 0.3},
}
SWITCHES = ("usePSPG", "useLSIC", "useSUPG", "transient", "incplanestress", "include advection")


class _PointOnMpf:
    """One point's coordinates as mpf under the indexing the point functions use: x.shape[2], x[..., d]."""

    def __init__(self, v):
        self.v, self.shape = v, (1, 1, len(v))

    def __getitem__(self, idx):
        return self.v[idx[-1]]


@pytest.mark.parametrize("module,dim", [(m, d) for m in H.LATER for d in (2, 3) if (m, d) != ("shallowwater", 3)])   # (a 2-D module)
def test_complex_step_matches_mpmath_diff_of_the_later_point_functions(module, dim):
    """C = dF/dU and dF/dUdot of every later module's point function by the complex step in clongdouble against mpmath.diff
    of the same expressions on mpf (the point functions are plain arithmetic: they run on mpf as they stand), at one point
    with every term switched on; cdr with the deck strings that read c, c_t, grad(c)[x] and ux."""
    S = 1 + dim
    nv = {"stokes": dim + 1, "shallowwater": 3, "helmholtz": 2, "cdr": 1, "linearelasticity+thermal": dim + 1}.get(module, dim + 2)
    K = nv * S
    rng = np.random.default_rng(17)
    U0, Ud0 = rng.uniform(-1, 1, K), rng.uniform(-1, 1, K)
    if module == "shallowwater":
        U0[0] = 0.8                                             # a depth xi + b well above 0
    x = np.array([0.25, 0.4, 0.15], LD)[:dim].reshape(1, 1, dim)
    P = dict(POINT_PARAMS[module])
    if "cdr" in module:
        P.update(_fields_of_c(module))
    U, Ud = U0.astype(LD).reshape(K, 1, 1), Ud0.astype(LD).reshape(K, 1, 1)
    F, CU, CT = H.point_derivative(H.POINT[module], U, Ud, x, dict(P, h=np.full((1, 1), LD(0.37))))

    with mpmath.workdps(40):
        Pm = {k: (mpmath.mpf(v) if isinstance(v, float) and k not in SWITCHES else v) for k, v in P.items()}
        Pm["h"] = mpmath.mpf(float(LD(0.37)))
        Um, Udm = [mpmath.mpf(float(v)) for v in U0], [mpmath.mpf(float(v)) for v in Ud0]
        xm = _PointOnMpf([mpmath.mpf(float(v)) for v in x[0, 0]])
        F_mp = lambda Uv, Udv: H.POINT[module](Uv, Udv, xm, Pm)
        Fm = F_mp(Um, Udm)
        assert len(Fm) == F.shape[0]
        scale = max(abs(f) for f in Fm)
        nonzero = 0
        for k in range(len(Fm)):
            assert abs(H._ld(Fm[k] + mpmath.mpf(0)) - F[k, 0, 0]) < 1e-18 * float(scale), k
            for l in range(K):
                def f(t, k=k, l=l):
                    return F_mp([u + (t if j == l else 0) for j, u in enumerate(Um)], Udm)[k] + mpmath.mpf(0)
                ref = mpmath.diff(f, 0)
                nonzero += ref != 0
                assert abs(H._ld(ref) - CU[k, l, 0, 0]) < 1e-17 * max(1.0, float(abs(ref))), (k, l, float(ref), float(CU[k, l, 0, 0]))
            for l in range(0, K, S):
                def g(t, k=k, l=l):
                    return F_mp(Um, [u + (t if j == l else 0) for j, u in enumerate(Udm)])[k] + mpmath.mpf(0)
                ref = mpmath.diff(g, 0)
                assert abs(H._ld(ref) - CT[k, l, 0, 0]) < 1e-17 * max(1.0, float(abs(ref))), (k, l)
        assert nonzero >= K                                     # (the comparison is not one of zeros)


def test_a_wrong_dof_ordering_is_a_gross_failure(oracle):
    c = H.build_case(oracle, "thermal", H.SHAPES["thermal"][1], "unit", False)
    m = dict(c["m"])
    off = m["offsets"].copy()
    off[[4, 5]] = off[[5, 4]]                                    # two basis functions trade their LID positions
    m["offsets"] = off
    with pytest.raises(AssertionError):
        H.Block(m, c["qdeg"], order=2).check_ordering()


def test_distance_leaves_no_entry_out():
    one = np.ones(3)
    assert H.distance([1.0, 1.0, 1.0 + 2.0 ** -50], one, one) == 8.0
    assert H.distance([1.0, np.nan, 1.0], one, one) == float("inf")           # a NaN is not a pass
    assert H.distance([1.0, np.inf, 1.0], one, one) == float("inf")
    assert H.distance([1.0, 1e-300, 1.0], [1.0, 0.0, 1.0], [1.0, 0.0, 1.0]) == float("inf")   # S == 0: exactly 0.0
    assert H.distance([1.0, np.nan, 1.0], [1.0, 0.0, 1.0], [1.0, 0.0, 1.0]) == float("inf")
    assert H.distance([1.0, 0.0, 1.0], [1.0, 0.0, 1.0], [1.0, 0.0, 1.0]) == 0.0


# ---- the oracle against the yardstick ---------------------------------------------------------------------------------------
def oracle_arrays(oracle, c):
    """local_J, local_res, crs_vals, res of the CPU oracle on the case's inputs."""
    m, P, tr, mod = c["m"], c["P"], c["tr"], c["module"]
    g = c["g"]
    if mod == "thermal" and c["family"] == "unit nonlinear":
        out = oracle.assemble_thermal_fields(c["dim"], c["orders"][0], c["qdeg"], m["nodes"], m["lids"], m["offsets"], c["u"],
                                             {"thermal source": H.sinprod_text(P["source"], c["dim"]),
                                              "thermal diffusion": P["diffusion_text"]}, fixed=c["fixed"],
                                             rowptr=g["rowptr"], colind=g["colind"])
    elif mod == "thermal":
        out = oracle.assemble_thermal(c["dim"], c["orders"][0], c["qdeg"], m["nodes"], m["lids"], m["offsets"], c["u"],
                                      fixed=c["fixed"], transient=tr, diff=P["diffusion"], rho=P["rho"], cp=P["cp"],
                                      source=P["source"], want_local=True, rowptr=g["rowptr"], colind=g["colind"],
                                      advection=P["adv"])
    elif mod == "navierstokes":
        funcs = {k: P[k] for k in ("source ux", "source uy", "source uz", "viscosity", "density")}
        out = oracle.assemble_block(m, oracle.PHYS_NAVIERSTOKES, c["qdeg"], c["u"], funcs=funcs,
                                    params=[P["useSUPG"], P["usePSPG"], P["fix_uz_offsets"]], fixed=c["fixed"], transient=tr,
                                    want_local=True, rowptr=g["rowptr"], colind=g["colind"])
    elif mod == "linearelasticity":
        import linearelasticity_ref as R
        funcs = {k: P[k] for k in ("lambda", "mu", "source dx", "source dy", "source dz")}
        out = R.assemble(oracle, m, c["qdeg"], c["u"], funcs=funcs, params=dict(incplanestress=P["incplanestress"]),
                         fixed=c["fixed"], transient=tr, rowptr=g["rowptr"], colind=g["colind"])
    else:
        out = later_oracle_arrays(oracle, c)
    return out


def later_oracle_arrays(oracle, c, **over):
    """The float64 restatements of the later point-engine modules (tests/*_ref.py on oracle_lib's tables) on the case's
    inputs.  over: functions / parameters to replace (the sensitivity test takes one term out with them)."""
    import importlib
    m, tr, mod, g = c["m"], c["tr"], c["module"], c["g"]
    funcs, params = H.deck(dict(c, P=dict(c["P"], **over)))
    R = importlib.import_module({"cdr": "cdr_ref", "navierstokes+cdr": "cdr_ref", "helmholtz": "helmholtz_ref", "stokes": "stokes_ref",
                                 "shallowwater": "shallowwater_ref", "navierstokes+thermal": "ns_thermal_ref",
                                 "linearelasticity+thermal": "thermoelastic_ref"}[mod])
    kw = dict(funcs=funcs, fixed=c["fixed"], transient=tr, rowptr=g["rowptr"], colind=g["colind"])
    if mod in ("stokes", "navierstokes+thermal", "linearelasticity+thermal"):
        kw["params"] = params
    if mod == "navierstokes+cdr":
        kw["ns_params"] = [params[k] for k in ("useSUPG", "usePSPG", "fix_uz_offsets")]
    return R.assemble(oracle, m, c["qdeg"], c["u"], **kw)


def distances(c, got):
    """d of the four arrays of `got` against the case's yardstick."""
    el, g = c["el"], c["g"]
    d = dict(crs_vals=H.distance(got["crs_vals"], g["crs_vals"], g["S_vals"]), res=H.distance(got["res"], g["res"], g["S_res"]))
    if "local_J" in got:
        d.update(local_J=H.distance(got["local_J"], el["local_J"], el["S_J"]),
                 local_res=H.distance(got["local_res"], el["local_res"], el["S_res"]))
    return d


MODULE_FAMILY = [(mod, fam) for mod in H.SHAPES for fam in H.families(mod)]


@pytest.mark.parametrize("module,family", MODULE_FAMILY)
def test_oracle_against_the_yardstick(oracle, module, family):
    """Every entry of the oracle's element arrays, CRS values and residual, every shape, steady and at stage 1.  This is
    the first pin of the oracle's Q2-hex thermal and 3-D Q2/Q1 navierstokes element arrays beyond 6 digits."""
    K = 0.0
    for shape, transient, variant in H.case_list(module, family):
        c = H.build_case(oracle, module, shape, family, transient, variant)
        assert np.array_equal(c["g"]["colind"], oracle.build_graph(c["m"]["ndof"], c["m"]["lids"])[1])
        if module in H.LATER:
            share = c["fixed"].mean()
            assert 0.10 <= share <= 0.30, ("the strong rows' share of all rows", c["tag"], share)
        d = distances(c, oracle_arrays(oracle, c))
        print("%-16s %-18s %-40s " % (module, family, c["tag"]) + "  ".join("%s %.3g" % kv for kv in d.items()))
        assert all(v == v for v in d.values()), d
        K = max(K, max(d.values()))
    rec = H.K_ORACLE.get((module, family))
    print("K_oracle[%s, %s] = %.4g (recorded %s, device bound %s)" %
          (module, family, K, rec, H.device_bound(module, family) if rec is not None else None))
    assert rec is not None, "no recorded K_oracle"
    assert K <= rec, "the oracle is farther from the yardstick than recorded"
    assert rec <= 1.5 * K + 1.0, "the recorded K_oracle is stale (more than half above the measurement)"


# ---- the bound is not slack: one term of a restatement off by a relative 2^-40 ----------------------------------------------
def _without(oracle, c, **over):
    return later_oracle_arrays(oracle, c, **over)


def _term(full, less):
    return {k: full[k] - less[k] for k in ("crs_vals", "res", "local_J", "local_res") if k in full}


def _buoyancy_pspg_part(oracle, c, full):
    """[PSPG on - off] with beta minus the same without: the undivided buoyancy part of the PSPG rows alone."""
    on0, off, off0 = _without(oracle, c, beta=0.0), _without(oracle, c, usePSPG=0), _without(oracle, c, usePSPG=0, beta=0.0)
    return {k: (full[k] - off[k]) - (on0[k] - off0[k]) for k in ("crs_vals", "res", "local_J", "local_res")}


ONE_TERM = {   # module -> (variant, what the term is, its contribution to the restatement's arrays)
    "stokes": (3, "the LSIC contribution", lambda o, c, full: _term(full, _without(o, c, useLSIC=0))),
    "shallowwater": (0, "g xi b_x", lambda o, c, full: _term(full, _without(o, c, bathymetry_x=0.0))),
    "helmholtz": (0, "the c2i_y direction", lambda o, c, full: _term(full, _without(o, c, c2i_y=0.0))),
    "cdr": (0, "xvel c_x", lambda o, c, full: _term(full, _without(o, c, xvel=0.0))),
    "navierstokes+cdr": (0, "xvel c_x", lambda o, c, full: _term(full, _without(o, c, xvel=0.0))),
    "navierstokes+thermal": (0, "the buoyancy part of PSPG", _buoyancy_pspg_part),
    "linearelasticity+thermal": (0, "alpha_T (e - T_ambient) in the normal stresses", lambda o, c, full: _term(full, _without(o, c, alpha_T=0.0))),
}


@pytest.mark.parametrize("module", H.LATER)
def test_one_term_off_by_2_to_the_minus_40_exceeds_the_device_bound(oracle, module):
    """ONE term of the float64 restatement's output, on the unit family, perturbed by a relative 2^-40 (8192 units of
    2^-53): the distance from the yardstick must exceed device_bound -- a device with that error in that term fails."""
    variant, what, term = ONE_TERM[module]
    bound = H.device_bound(module, "unit")
    for transient in (False, True):
        c = H.build_case(oracle, module, H.SHAPES[module][0], "unit", transient, variant)
        full = later_oracle_arrays(oracle, c)
        t = term(oracle, c, full)
        assert max(np.abs(v).max() for v in t.values()) > 0, what
        clean, off = distances(c, full), distances(c, {k: full[k] + 2.0 ** -40 * t[k] for k in t})
        print("%-26s %-48s %-8s d %.3g -> %.3g  (bound %.3g)" % (module, what, "stage 1" if transient else "steady",
                                                                   max(clean.values()), max(off.values()), bound))
        assert max(clean.values()) <= bound < max(off.values()), (what, clean, off, bound)
