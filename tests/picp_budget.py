"""The PICP linearisation in plain numpy with a first-order error budget.  Test infrastructure only.

system() restates what one round of the solver sums -- H = sum(lambda J^T J), b = sum(lambda J^T e), the chi^2 sums and the
inlier count -- from the formulas (the same ones tests/np_restatement.py::linearize evaluates with matrix products; here they
are written entry by entry so that the SAME code also runs in float32, every operation rounded once, and so that each factor
can be replaced by its absolute value).  With dt = float64 it is the reference value; with dt = float32 it is "the
reference's formulas in float32 with numpy's pairwise sums", the arithmetic the ceiling C is measured on.

Budgets.  A_X is the formula of X with every factor replaced by its absolute value, summed over the correspondences that
contribute: a first-order bound of what ONE relative rounding of 2^-24 in every factor can move X by, whatever the
summation order.  Two factors need more than |value|:
  * e = uv - z loses ulps of the PIXEL (uv and z are ~hundreds, e is ~1): it carries |uv| + |z|;
  * for a kept outlier lambda = sqrt(thr / chi) inherits chi's relative error 2 (|uv| + |z|) . |e| / chi, halved by the
    square root: its weight carries the factor 1 + (|uv| + |z|) . |e| / chi.
rho(X) = max over entries |X_got - X64| / (2^-24 A_X) is then a small constant for any correct float32 evaluation --
about the number of roundings on the longest chain -- independent of n and of the pose.  An entry whose budget is exactly 0
has only structurally zero terms and must be exactly 0.

Ambiguous correspondences.  The default arithmetic may decide a gate either way for a correspondence whose float64 value
lies within the bands tests/test_gpu_gates.py holds (BAND below, in float32 ulps of the gate; of the principal point / of 1
where the gate is 0).  Those correspondences are returned with everything each of them contributes under each decision open
to it (gated out / inlier / outlier), and their own term magnitudes join the budgets.  A result is held to the float64 sums
under ONE decision of them all -- the same for H, b, the chi^2 sums and the inlier count (rho_system tries every combination,
combos) -- which keeps the check as sharp as without them: one whole term is hundreds of times the rounding budget of a
sum.  Only beyond 2^16 combinations do absolute allowances E_X (the largest change each can cause, not scaled by C) stand
in, and n_in may then differ by their count.  A case may hold at most amb_cap(n) of them.

One Gauss-Newton step.  step() solves (H64 + I) dx = -b64 and bounds dx entry by entry:
  |H^-1| (tol_b + tol_H |dx|) + C_LDLT 2^-24 |H^-1| (|R^T| |R|) |dx|,   tol_X = C 2^-24 A_X (+ E_X),
R the Cholesky factor of H64 + I: a 6x6 LDL^T / Cholesky solve has the backward error gamma_(3n+1) |R^T| |R| (Higham,
Accuracy and Stability, thm 10.4), 3n + 1 = 19 = C_LDLT.  dx of a GPU pose is read off T_out T0^-1 (dx_of); the pose
composition's own rounding -- sin / cos (2 ulp), Rx Ry Rz (two products and an add per entry: 3), the 3-term product with T0
and the added translation (4) -- is C_POSE = 9 roundings of |v2t(dx)| |T0| per entry of T_out, carried through |T0^-1| and
through the derivatives of the angle extraction.

The tail alone.  A solver that returns the float32 H (damping included) and b it solved is held more sharply: tail() is the
same step with tol_H = tol_b = 0 -- the float64 solution of THAT system composed with the pose before the round, bounded by
the LDL^T and composition terms only, no sum over correspondences in it (check_tail; ceiling: picp_cases.ceiling_tail).
tail32() restates the tail in float32, one rounding per operation, and takes planted faults (TAIL_FAULTS)."""
import numpy as np

from np_restatement import v2t_euler

U = 2.0 ** -24
BAND = dict(depth=4, image=8, chi=1024)          # tests/test_gpu_gates.py: BAND
C_LDLT = 19.0
C_POSE = 9.0
N_CU = 256                                       # MI355X; the GPU test asserts the device reports the same
SLOT = [(r, c) for r in range(6) for c in range(r, 6)]        # the 21 accumulators: upper triangle row by row (vo_math.h)
VALUE_FAULTS = ("sign", "world_point", "lambda_one", "slot")
COVERAGE_FAULTS = ("drop_last_inlier", "drop_block", "double_block")


def amb_cap(n):
    return max(2, int(np.floor(0.0002 * n)))


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x) if x != 0 else 1.0)))


def _jacobian(iz, g0, g1, K, p, absval):
    """J = (Jp K) [I | skew(-p)], rows J0, J1 as lists of six arrays.  Jp = [iz 0 g0; 0 iz g1].  absval: every factor
    replaced by its absolute value (the caller passes absolute iz, g, K, p), differences become sums."""
    s = 1.0 if absval else -1.0
    A = []
    for g, row in ((g0, 0), (g1, 1)):
        A.append([iz * K[row, c] + g * K[2, c] for c in range(3)])
    J = []
    for a in A:
        # skew(v), v = -p: [0 -v2 v1; v2 0 -v0; -v1 v0 0]  ->  columns 3..5 of [I | skew(-p)] are (0, -p2, p1), (p2, 0, -p0), (-p1, p0, 0)
        J.append([a[0], a[1], a[2],
                  a[1] * (s * p[2]) + a[2] * p[1],
                  a[0] * p[2] + a[2] * (s * p[0]),
                  a[0] * (s * p[1]) + a[1] * p[0]])
    return J


def _colsum(cols, dt):
    """sum each of a list of (n,) arrays in dt; float32 goes through numpy's pairwise summation of a contiguous row"""
    return np.array([np.ascontiguousarray(c).sum(dtype=dt) for c in cols], dtype=dt)


def system(K, T, world, meas, corr, thr, keep_outliers, rows, cols, z_near, z_far, dt=np.float64, fault=None):
    """-> dict: H (6x6, no damping), b, chi_in, chi_out, n_in in dt arithmetic; for dt = float64 also the budgets A_H, A_b,
    A_chi_in, A_chi_out, the ambiguous correspondences `amb` (indices into corr) and their allowances E_H, E_b, E_chi_in,
    E_chi_out.  `fault` plants one of VALUE_FAULTS / COVERAGE_FAULTS."""
    dt = np.dtype(dt).type
    corr = np.asarray(corr, np.int32).reshape(-1, 2)
    K = np.asarray(K, dt); T = np.asarray(T, dt)
    thr = dt(thr)
    n = len(corr)
    pw = np.asarray(world, dt)[corr[:, 1]].reshape(n, 3)
    z = np.asarray(meas, dt)[corr[:, 0]].reshape(n, 2)
    w = [pw[:, 0], pw[:, 1], pw[:, 2]]
    with np.errstate(all="ignore"):
        pc = [T[i, 3] + (T[i, 0] * w[0] + (T[i, 1] * w[1] + T[i, 2] * w[2])) for i in range(3)]
        ph = [K[i, 0] * pc[0] + (K[i, 1] * pc[1] + K[i, 2] * pc[2]) for i in range(3)]
        iz = dt(1) / ph[2]
        u, v = ph[0] * iz, ph[1] * iz
        ok = ~((pc[2] > z_far) | (pc[2] < z_near))
        ok &= ~((u < 0) | (u > cols - 1) | (v < 0) | (v > rows - 1))
        e0, e1 = u - z[:, 0], v - z[:, 1]
        chi = e0 * e0 + e1 * e1
        outl = ok & (chi > thr)
        inl = ok & ~(chi > thr)
        iz2 = iz * iz
        g0, g1 = -ph[0] * iz2, -ph[1] * iz2
        p = w if fault == "world_point" else pc
        J0, J1 = _jacobian(iz, g0, g1, K, p, False)
        if fault == "sign":
            J0[3] = J0[3] - 2 * (J0[2] * p[1]); J1[3] = J1[3] - 2 * (J1[2] * p[1])      # skew entry (2, 3) negated
        lam = np.where(outl, np.sqrt(thr / chi), dt(1)).astype(dt)
    if fault == "lambda_one":
        lam = np.ones_like(lam)
    mult = np.ones(n, np.int64)                           # how often a correspondence is visited: coverage faults
    if fault == "drop_last_inlier":
        mult[np.nonzero(inl)[0][-1]] = 0
    elif fault == "drop_block":
        mult[max(0, n - 256):] = 0
    elif fault == "double_block":
        mult[max(0, n - 256):] = 2
    use = (inl | (outl & bool(keep_outliers))) & (mult > 0)
    wgt = np.where(use, lam, dt(0)).astype(dt) * mult.astype(dt)
    with np.errstate(all="ignore"):
        hs = _colsum([np.where(use, (J0[r] * J0[c] + J1[r] * J1[c]) * wgt, dt(0)) for r, c in SLOT], dt)
        bs = _colsum([np.where(use, (J0[r] * e0 + J1[r] * e1) * wgt, dt(0)) for r in range(6)], dt)
        chi_in = _colsum([np.where(inl, chi, dt(0)) * mult.astype(dt)], dt)[0]
        chi_out = _colsum([np.where(outl, chi, dt(0)) * mult.astype(dt)], dt)[0]
    H = np.zeros((6, 6), dt)
    for k, (r, c) in enumerate(SLOT):
        if fault == "slot" and (r, c) == (1, 3):
            k += 1                                        # entry (1, 3) read from the slot of (1, 4)
        H[r, c] = H[c, r] = hs[k]
    out = dict(H=H, b=bs, chi_in=chi_in, chi_out=chi_out, n_in=int((inl * mult).sum()), n_out=int((outl * mult).sum()))
    if dt is not np.float64:
        return out
    # ---- budgets: the same formulas, every factor by its absolute value --------------------------------------------------
    aK = np.abs(K)
    with np.errstate(all="ignore"):
        A0, A1 = _jacobian(np.abs(iz), np.abs(g0), np.abs(g1), aK, [np.abs(x) for x in p], True)
        ea0, ea1 = np.abs(u) + np.abs(z[:, 0]), np.abs(v) + np.abs(z[:, 1])
        ae0, ae1 = np.abs(e0), np.abs(e1)
        wa = np.where(outl, 1.0 + (ea0 * ae0 + ea1 * ae1) / chi, 1.0) * np.abs(wgt)
        ah = [np.where(use, (A0[r] * A0[c] + A1[r] * A1[c]) * wa, 0.0).sum() for r, c in SLOT]
        A_b = np.array([np.where(use, (A0[r] * ea0 + A1[r] * ea1) * wa, 0.0).sum() for r in range(6)])
        achi = 2 * (ea0 * ae0 + ea1 * ae1) + chi
        A_ci = float(np.where(inl & (mult > 0), achi, 0.0).sum())
        A_co = float(np.where(outl & (mult > 0), achi, 0.0).sum())
        # ---- ambiguous correspondences: float64 value inside a band around a gate ---------------------------------------
        gate = np.abs(pc[2] - z_far) <= BAND["depth"] * _ulp32(z_far)
        gate |= np.abs(pc[2] - z_near) <= BAND["depth"] * _ulp32(z_near)
        gate |= np.abs(u) <= BAND["image"] * _ulp32(K[0, 2])
        gate |= np.abs(u - (cols - 1)) <= BAND["image"] * _ulp32(cols - 1)
        gate |= np.abs(v) <= BAND["image"] * _ulp32(K[1, 2])
        gate |= np.abs(v - (rows - 1)) <= BAND["image"] * _ulp32(rows - 1)
        wchi = BAND["chi"] * _ulp32(thr)
        edge = (ok | gate) & (np.abs(chi - thr) <= wchi)
        amb = np.nonzero(gate | edge)[0]
        # everything an ambiguous correspondence can contribute, in either decision: [21 H slots, 6 b, chi_in, chi_out, n_in]
        tH = np.stack([(J0[r][amb] * J0[c][amb] + J1[r][amb] * J1[c][amb]) for r, c in SLOT], 1).reshape(len(amb), 21)
        tb = np.stack([J0[r][amb] * e0[amb] + J1[r][amb] * e1[amb] for r in range(6)], 1).reshape(len(amb), 6)
        aH = np.stack([(A0[r][amb] * A0[c][amb] + A1[r][amb] * A1[c][amb]) for r, c in SLOT], 1).reshape(len(amb), 21)
        ab = np.stack([A0[r][amb] * ea0[amb] + A1[r][amb] * ea1[amb] for r in range(6)], 1).reshape(len(amb), 6)
    alts, E = [], np.zeros(30)
    for j, i in enumerate(amb):
        lo = float(lam[i]) if keep_outliers else 0.0           # weight as an outlier
        m = float(mult[i])

        def contrib(state):                                     # 0 gated out, 1 inlier, 2 outlier
            if state == 0:
                return np.zeros(30)
            if state == 1:
                return m * np.concatenate([tH[j], tb[j], [chi[i], 0.0, 1.0]])
            return m * np.concatenate([lo * tH[j], lo * tb[j], [0.0, chi[i], 0.0]])
        now = 0 if not ok[i] else (2 if outl[i] else 1)
        by_chi = {1, 2} if edge[i] else ({2} if chi[i] > thr else {1})
        states = (by_chi | {0}) if gate[i] else by_chi
        d = [contrib(s) - contrib(now) for s in sorted(states) if s != now]
        alts.append(d)
        E += np.abs(np.array(d)).max(0)
        # their own term magnitudes join the budgets: whichever way the decision goes, the term carries its roundings, and a
        # lambda taken on the other side of the threshold is 1 to within BAND["chi"] roundings
        k = 1.0 + (BAND["chi"] if edge[i] and keep_outliers else 0.0)
        ah = list(np.asarray(ah) + m * k * aH[j]); A_b = A_b + m * k * ab[j]
        A_ci += m * float(achi[i]); A_co += m * float(achi[i])       # (on the side it already is on: counted twice, harmless)
    A_H = np.zeros((6, 6)); E_H = np.zeros((6, 6))
    for k, (r, c) in enumerate(SLOT):
        A_H[r, c] = A_H[c, r] = ah[k]
        E_H[r, c] = E_H[c, r] = E[k]
    out.update(A_H=A_H, A_b=A_b, A_chi_in=A_ci, A_chi_out=A_co, amb=amb, n_amb=len(amb), alts=alts,
               E_H=E_H, E_b=E[21:27], E_chi_in=float(E[27]), E_chi_out=float(E[28]), n=n)
    return out


def combos(ref, limit=1 << 16):
    """every way the ambiguous correspondences can be decided, as differences from the float64 decisions: (m, 30) rows of
    [21 H slots, 6 b, chi_in, chi_out, n_in], row 0 all zero.  None when there are more than `limit` (the caller then falls
    back on the allowances E_X)."""
    D = np.zeros((1, 30))
    for d in ref["alts"]:
        if not d:
            continue
        if len(D) * (len(d) + 1) > limit:
            return None
        D = (D[:, None, :] + np.concatenate([np.zeros((1, 30)), np.array(d)])[None, :, :]).reshape(-1, 30)
    return D


def _pack(H, b, chi_in, chi_out):
    H = np.asarray(H, np.float64)
    return np.concatenate([[H[r, c] for r, c in SLOT], np.asarray(b, np.float64), [float(chi_in), float(chi_out)]])


def _unpack_H(vec):
    H = np.zeros((6, 6))
    for k, (r, c) in enumerate(SLOT):
        H[r, c] = H[c, r] = vec[k]
    return H


def rho(X, X64, A, E=0.0):
    """max over entries of (|X - X64| - E) / (2^-24 A); inf if an entry with a zero budget (and no allowance) is not exactly
    X64's"""
    X = np.asarray(X, np.float64); X64 = np.asarray(X64, np.float64); A = np.asarray(A, np.float64)
    d = np.maximum(np.abs(X - X64) - E, 0.0) + np.zeros_like(A)
    if not np.isfinite(d).all():
        return float("inf")
    z = A == 0
    if (d[z] != 0).any():
        return float("inf")
    return float((d[~z] / (U * A[~z])).max()) if (~z).any() else 0.0


def rho_system(ref, H, b, chi_in, chi_out, n_in=None, damping=0.0):
    """the statistic of a whole system against system()'s float64 result `ref`: dict(H, b, chi_in, chi_out, worst, n_in_ok,
    delta).  H holds the damping the solver leaves on its diagonal (one more rounding at the magnitude of sum + damping: the
    diagonal budget gets it too).
    The ambiguous correspondences are decided ONE way for all of H, b, the chi^2 sums and the count together: every
    combination of their decisions (combos) whose inlier count is the given n_in is tried and the one with the smallest
    worst entry reported -- `delta` is its row.  With more combinations than combos() enumerates, the allowances E_X stand
    in and n_in may differ by the number of ambiguous correspondences."""
    H = np.asarray(H, np.float64)
    Dg = damping * np.eye(6)
    got = _pack(np.triu(H) , b, chi_in, chi_out)
    low = _pack(np.tril(H).T, b, chi_in, chi_out)          # the lower triangle is held to the same values
    want = _pack(ref["H"] + Dg, ref["b"], ref["chi_in"], ref["chi_out"])
    A = _pack(ref["A_H"] + Dg, ref["A_b"], ref["A_chi_in"], ref["A_chi_out"])
    D = combos(ref)
    dn = None if n_in is None else int(n_in) - ref["n_in"]
    if D is None:
        E = _pack(ref["E_H"], ref["E_b"], ref["E_chi_in"], ref["E_chi_out"])
        r = [max(rho(got[s], want[s], A[s], E[s]), rho(low[s], want[s], A[s], E[s])) for s in (slice(0, 21), slice(21, 27), slice(27, 28), slice(28, 29))]
        return dict(H=r[0], b=r[1], chi_in=r[2], chi_out=r[3], worst=max(r), n_in_ok=dn is None or abs(dn) <= ref["n_amb"], delta=None)
    if dn is not None:
        D = D[D[:, 29] == dn]
    if len(D) == 0:
        inf = float("inf")
        return dict(H=inf, b=inf, chi_in=inf, chi_out=inf, worst=inf, n_in_ok=False, delta=None)
    with np.errstate(all="ignore"):
        d = np.maximum(np.abs(got[None, :] - (want[None, :] + D[:, :29])), np.abs(low[None, :] - (want[None, :] + D[:, :29])))
        r = np.where(A[None, :] > 0, d / (U * np.where(A > 0, A, 1.0))[None, :], np.where(d == 0, 0.0, np.inf))
        r = np.where(np.isfinite(d), r, np.inf)
    k = int(np.argmin(r.max(1)))
    r = r[k]
    return dict(H=float(r[:21].max()), b=float(r[21:27].max()), chi_in=float(r[27]), chi_out=float(r[28]), worst=float(r.max()),
                n_in_ok=True, delta=D[k])


def _solve_bounds(Hd, b, T0):
    """what step() and tail() share: dx = Hd^-1 (-b) in float64, |Hd^-1|, the LDL^T backward-error term and the pose
    composition's term of the bound (module docstring), T1 = v2t(dx) T0"""
    T0 = np.asarray(T0, np.float64)
    dx = np.linalg.solve(Hd, -b)
    Hi = np.abs(np.linalg.inv(Hd))
    R = np.linalg.cholesky(Hd).T
    adx = np.abs(dx)
    tol_ldlt = C_LDLT * U * (Hi @ ((np.abs(R.T) @ np.abs(R)) @ adx))
    dT = v2t_euler(dx)
    # what the composition's own rounding moves dx_of(T_out, T0) by
    E_T = C_POSE * U * (np.abs(dT) @ np.abs(T0))
    E_dT = E_T @ np.abs(np.linalg.inv(T0))
    cy = max(abs(np.cos(dx[4])), 1e-3)
    ext = np.array([E_dT[0, 3], E_dT[1, 3], E_dT[2, 3], (E_dT[1, 2] + E_dT[2, 2]) / cy, E_dT[0, 2] / cy,
                    (E_dT[0, 1] + E_dT[0, 0]) / cy])
    return dict(dx=dx, adx=adx, Hi=Hi, T1=dT @ T0, tol_ldlt=tol_ldlt, tol_pose=ext)


def step(ref, T0, C, delta=None):
    """one damped Gauss-Newton step from system()'s float64 result: dx64, T1_64 = v2t(dx64) T0 and the entrywise bound of dx
    for an evaluation that keeps rho <= C.  delta: a row of combos() -- the ambiguous correspondences decided that way, no
    allowance; None: the float64 decisions with the allowances E_X."""
    H, b = ref["H"], ref["b"]
    E_H, E_b = ref["E_H"], ref["E_b"]
    if delta is not None:
        H = H + _unpack_H(delta); b = b + delta[21:27]
        E_H, E_b = 0.0, 0.0
    s = _solve_bounds(H + np.eye(6), b, T0)
    tol_H = C * U * (ref["A_H"] + np.eye(6)) + E_H
    tol_b = C * U * ref["A_b"] + E_b
    tol = s["Hi"] @ (tol_b + tol_H @ s["adx"]) + s["tol_ldlt"]
    return dict(dx=s["dx"], T1=s["T1"], tol=tol + s["tol_pose"], tol_system=tol, tol_pose=s["tol_pose"])


def tail(H32, b32, T_at):
    """the solver's tail as a pure function of the float32 system it solved (H with the damping on its diagonal, b:
    vo_picp_get_system) and the pose before the round: the float64 step dx = H^-1 (-b), T1 = v2t(dx) T_at, and what is left
    of step()'s bound when H and b are exact (tol_H = tol_b = 0) -- the LDL^T backward error and the composition's
    roundings.  No sum over correspondences is in it."""
    s = _solve_bounds(np.asarray(H32, np.float64), np.asarray(b32, np.float64), T_at)
    return dict(dx=s["dx"], T1=s["T1"], tol=s["tol_ldlt"] + s["tol_pose"], tol_ldlt=s["tol_ldlt"], tol_pose=s["tol_pose"])


def check_tail(H32, b32, T_at, T_out):
    """-> max |dx_of(T_out, T_at) - dx64| / tail()'s bound; inf for a pose that is not finite"""
    t = tail(H32, b32, T_at)
    if not np.isfinite(np.asarray(T_out, np.float64)).all():
        return float("inf")
    d = np.abs(dx_of(T_out, T_at) - t["dx"])
    with np.errstate(all="ignore"):
        r = np.where(t["tol"] > 0, d / t["tol"], np.where(d == 0, 0.0, np.inf))
    return float(np.max(r)) if np.isfinite(r).all() else float("inf")


TAIL_FAULTS = ("swap_angles", "compose_order", "drop_translation", "recip_17ulp", "poly_everywhere", "stale_pose", "b_sign")


def _sincos_poly32(x):
    """csrc/vo_math.h sincos_small with every operation rounded once (no FMA)"""
    f = np.float32
    z = x * x
    ps = f(-1.9515295891e-4) * z + f(8.3321608736e-3)
    ps = ps * z + f(-1.6666654611e-1)
    s = (ps * z) * x + x
    pc = f(2.443315711809948e-5) * z + f(-1.388731625493765e-3)
    pc = pc * z + f(4.166664568298827e-2)
    c = (pc * z) * z + (f(-0.5) * z + f(1.0))
    return f(s), f(c)


def tail32(H32, b32, T_at, fault=None, T_prev=None):
    """the tail in float32, one rounding per operation, written out like system(dt=float32): LDL^T of H in the natural
    order without pivoting (unfused products, a true division for each pivot's reciprocal), forward / diagonal / backward
    substitution of -b, float32 sin / cos, R = Rx Ry Rz, T_out = v2t(dx) T_at with 3-term products and the translation added
    last.  -> T_out (4x4 float32).  `fault` plants one of TAIL_FAULTS; stale_pose composes with T_prev, the pose one round
    older."""
    f = np.float32
    assert fault is None or fault in TAIL_FAULTS, fault
    B = np.array(H32, f).reshape(6, 6).copy()
    b = np.asarray(b32, f)
    y = [b[i] if fault == "b_sign" else -b[i] for i in range(6)]
    T = np.array(T_prev if fault == "stale_pose" else T_at, f).reshape(4, 4)
    inv = [f(0)] * 6
    with np.errstate(all="ignore"):
        for k in range(6):
            if k > 0:
                tmp = [B[j, j] * B[k, j] for j in range(k)]
                acc = f(0)
                for j in range(k):
                    acc = acc + B[k, j] * tmp[j]
                B[k, k] = B[k, k] - acc
                for i in range(k + 1, 6):
                    acc = f(0)
                    for j in range(k):
                        acc = acc + B[i, j] * tmp[j]
                    B[i, k] = B[i, k] - acc
            inv[k] = f(1) / B[k, k] if abs(B[k, k]) > f(1.17549435e-38) else f(0)
            if fault == "recip_17ulp":
                inv[k] = inv[k] * f(1 + 2e-6)
            for i in range(k + 1, 6):
                B[i, k] = B[i, k] * inv[k]
        for i in range(1, 6):
            for j in range(i):
                y[i] = y[i] - B[i, j] * y[j]
        for i in range(6):
            y[i] = y[i] * inv[i]
        for i in range(4, -1, -1):
            for j in range(i + 1, 6):
                y[i] = y[i] - B[j, i] * y[j]
        ax, ay, az = (y[4], y[3], y[5]) if fault == "swap_angles" else (y[3], y[4], y[5])
        if fault == "poly_everywhere":
            (sx, cx), (sy, cy), (sz, cz) = _sincos_poly32(ax), _sincos_poly32(ay), _sincos_poly32(az)
        else:
            sx, cx, sy, cy, sz, cz = np.sin(ax), np.cos(ax), np.sin(ay), np.cos(ay), np.sin(az), np.cos(az)
        # Rx Ry = [cy 0 sy; sx sy  cx  -sx cy; -cx sy  sx  cx cy], then times Rz (structural zeros and ones dropped: exact)
        a10, a12, a20, a22 = sx * sy, -sx * cy, -cx * sy, cx * cy
        dT = np.eye(4, dtype=f)
        dT[0, :3] = [cy * cz, cy * -sz, sy]
        dT[1, :3] = [a10 * cz + cx * sz, a10 * -sz + cx * cz, a12]
        dT[2, :3] = [a20 * cz + sx * sz, a20 * -sz + sx * cz, a22]
        dT[:3, 3] = y[:3]
        A, Bm = (T, dT) if fault == "compose_order" else (dT, T)
        out = np.eye(4, dtype=f)
        for r in range(3):
            for c in range(4):
                e = A[r, 0] * Bm[0, c] + (A[r, 1] * Bm[1, c] + A[r, 2] * Bm[2, c])
                if c == 3 and fault != "drop_translation":
                    e = e + A[r, 3]
                out[r, c] = e
    return out


def dx_of(T_out, T0):
    """the step a pose update T_out = v2t(dx) T0 took: translation dx[:3], angles from R = Rx Ry Rz (np_restatement.v2t_euler)"""
    D = np.asarray(T_out, np.float64) @ np.linalg.inv(np.asarray(T0, np.float64))
    R = D[:3, :3]
    return np.array([D[0, 3], D[1, 3], D[2, 3], np.arctan2(-R[1, 2], R[2, 2]), np.arcsin(np.clip(R[0, 2], -1, 1)),
                     np.arctan2(-R[0, 1], R[0, 0])])


def check_step(ref, T0, T_out, stats, C):
    """a solver that returns no H and b, held through its one-step pose: -> dict(stats = rho of the chi^2 sums (and the count
    matched exactly) for the best decision of the ambiguous correspondences, ratio = max |dx_got - dx64| / bound for that
    decision (<= 1 passes), dx, dx_got).  Every decision consistent with the returned statistics is tried."""
    dxg = dx_of(T_out, T0)
    D = combos(ref)
    cands = [None]
    if D is not None:
        cands = [d for d in D[D[:, 29] == int(round(float(stats[2]))) - ref["n_in"]]]
    best = None
    for d in cands:
        ci, co = ref["chi_in"] + (0.0 if d is None else d[27]), ref["chi_out"] + (0.0 if d is None else d[28])
        rs = max(rho(stats[0], ci, ref["A_chi_in"], ref["E_chi_in"] if d is None else 0.0),
                 rho(stats[1], co, ref["A_chi_out"], ref["E_chi_out"] if d is None else 0.0))
        st = step(ref, T0, C, d)
        with np.errstate(all="ignore"):
            ratio = float(np.max(np.where(st["tol"] > 0, np.abs(dxg - st["dx"]) / st["tol"], np.where(dxg == st["dx"], 0.0, np.inf))))
        key = max(rs / C, ratio)
        if best is None or key < best["key"]:
            best = dict(key=key, stats=rs, ratio=ratio, dx=st["dx"], dx_got=dxg, tol=st["tol"])
    if best is None:
        inf = float("inf")
        best = dict(key=inf, stats=inf, ratio=inf, dx=None, dx_got=dxg, tol=None)
    if D is None:
        best["n_in_ok"] = abs(int(round(float(stats[2]))) - ref["n_in"]) <= ref["n_amb"]
    else:
        best["n_in_ok"] = len(cands) > 0
    return best
