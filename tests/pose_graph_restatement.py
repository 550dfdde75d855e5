"""NumPy restatement of voe_pose_graph* (include/vo_pose_graph.h), written from the header's rules, in float64: the similarity
algebra, the residual of an edge and its two Jacobians as explicit 7x7 matrices, the Levenberg-Marquardt round with its PCG
and both preconditioners, the accept rule, the statuses and what is written.  It follows the header, not the kernels: the
Jacobians are matrices here and functions there, the chain's sums run frame by frame here and by doubling steps there, so the two
agree to rounding and not bit for bit.  `reverse` takes every sum over edges in the opposite order (the budget's second run);
`fault` plants one wrong reading of the header (FAULTS) that the GPU test's measure must see; solver="dense" replaces the PCG
by a plain dense solve of the same damped system, which is used only to show where the PCG lands."""
import numpy as np

STATUS = ("OK", "NOT_FINITE", "NOTHING_FREE", "NO_EDGES", "NO_STEP", "COST_ROSE")
PRECONDITIONER = ("CHAIN", "JACOBI")
EDGE_OK, EDGE_SKIPPED = 0, 1
ACTIVE, HELD, ISOLATED = 0, 1, 2
DEFAULT = dict(n_rounds=8, n_cg=8, cg_tol=1e-6, lambda0=1e-4, huber=0.0, with_scale=True, preconditioner="CHAIN")
FAULTS = ("ad_sign", "g_without_scale", "right_update", "no_irls", "no_damping", "accept_always", "chain_no_restart",
          "round_every_round", "z_inverted")


# ---- batched 3x3 and similarity algebra ----
def det3(M):
    return (M[..., 0, 0] * (M[..., 1, 1] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 1])
            - M[..., 0, 1] * (M[..., 1, 0] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 0])
            + M[..., 0, 2] * (M[..., 1, 0] * M[..., 2, 1] - M[..., 1, 1] * M[..., 2, 0]))


def inv3(M):
    """the adjugate over the determinant"""
    d = det3(M)
    A = np.empty_like(M)
    A[..., 0, 0] = M[..., 1, 1] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 1]
    A[..., 0, 1] = M[..., 0, 2] * M[..., 2, 1] - M[..., 0, 1] * M[..., 2, 2]
    A[..., 0, 2] = M[..., 0, 1] * M[..., 1, 2] - M[..., 0, 2] * M[..., 1, 1]
    A[..., 1, 0] = M[..., 1, 2] * M[..., 2, 0] - M[..., 1, 0] * M[..., 2, 2]
    A[..., 1, 1] = M[..., 0, 0] * M[..., 2, 2] - M[..., 0, 2] * M[..., 2, 0]
    A[..., 1, 2] = M[..., 0, 2] * M[..., 1, 0] - M[..., 0, 0] * M[..., 1, 2]
    A[..., 2, 0] = M[..., 1, 0] * M[..., 2, 1] - M[..., 1, 1] * M[..., 2, 0]
    A[..., 2, 1] = M[..., 0, 1] * M[..., 2, 0] - M[..., 0, 0] * M[..., 2, 1]
    A[..., 2, 2] = M[..., 0, 0] * M[..., 1, 1] - M[..., 0, 1] * M[..., 1, 0]
    with np.errstate(all="ignore"):
        return A / d[..., None, None]


def sim_inv(M, t):
    Mi = inv3(M)
    return Mi, -np.einsum("...ij,...j->...i", Mi, t)


def sim_mul(Ma, ta, Mb, tb):
    return Ma @ Mb, np.einsum("...ij,...j->...i", Ma, tb) + ta


def log_so3(R):
    v = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1) / 2.0
    n = np.sqrt((v * v).sum(-1))
    theta = np.arctan2(n, (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0) / 2.0)
    with np.errstate(all="ignore"):
        k = np.where(theta < 1e-4, 1.0 + theta * theta / 6.0, theta / n)
    return v * k[..., None]


def skew(t):
    S = np.zeros(t.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -t[..., 2], t[..., 1]
    S[..., 1, 0], S[..., 1, 2] = t[..., 2], -t[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -t[..., 1], t[..., 0]
    return S


def ad_matrices(M, t):
    """Ad([c R | t]) and its inverse written with R^T for R^-1 and R^T / c for M^-1, as 7x7 matrices"""
    with np.errstate(all="ignore"):
        c = np.cbrt(det3(M))
        R = M / c[..., None, None]
    n = M.shape[:-2]
    A, Ai = np.zeros(n + (7, 7)), np.zeros(n + (7, 7))
    tx = skew(t)
    Rt = np.swapaxes(R, -1, -2)
    A[..., :3, :3], A[..., :3, 3:6], A[..., :3, 6] = M, tx @ R, -t
    A[..., 3:6, 3:6] = R
    A[..., 6, 6] = 1.0
    with np.errstate(all="ignore"):
        Ai[..., :3, :3] = Rt / c[..., None, None]
        Ai[..., :3, 3:6] = -(Rt @ tx) / c[..., None, None]
        Ai[..., :3, 6] = np.einsum("...ij,...j->...i", Rt, t) / c[..., None]
    Ai[..., 3:6, 3:6] = Rt
    Ai[..., 6, 6] = 1.0
    return A, Ai


def g_matrix(tE, fault=None):
    G = np.zeros(tE.shape[:-1] + (7, 7))
    G[..., np.arange(7), np.arange(7)] = 1.0
    G[..., :3, 3:6] = -skew(tE)
    if fault != "g_without_scale":
        G[..., :3, 6] = tE
    return G


def rot_xyz(w):
    sx, cx, sy, cy, sz, cz = np.sin(w[0]), np.cos(w[0]), np.sin(w[1]), np.cos(w[1]), np.sin(w[2]), np.cos(w[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def apply_update(M, t, x, with_scale, fault=None):
    """S <- [e^sigma Rx Ry Rz | tau] S"""
    es = np.exp(x[6]) if with_scale else 1.0
    D = es * rot_xyz(x[3:6])
    if fault == "right_update":
        return M @ D, M @ x[:3] + t
    return D @ M, D @ t + x[:3]


def tree_sum(values):
    """item k into partial sum k mod 256 in item order, the 256 partial sums by a binary tree"""
    s = np.zeros(256)
    for k, v in enumerate(values):
        s[k % 256] += v
    h = 128
    while h >= 1:
        s[:h] += s[h:2 * h]
        h //= 2
    return s[0]


def mats(S):
    S = np.asarray(S, np.float64).reshape(-1, 4, 4)
    return S[:, :3, :3].copy(), S[:, :3, 3].copy()


# ---- the edges at a state ----
def live_edges(F, edges, weights):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    E = len(e)
    w = np.ones((E, 3)) if weights is None else np.asarray(weights, np.float32).astype(np.float64).reshape(E, 3)
    with np.errstate(all="ignore"):
        ok = (e[:, 0] >= 0) & (e[:, 0] < F) & (e[:, 1] >= 0) & (e[:, 1] < F) & (e[:, 0] != e[:, 1])
        ok &= np.all(np.isfinite(w) & (w >= 0), 1) & np.any(w > 0, 1)
    return e, w, ok


def evaluate(M, t, e, Zm, Zt, w3, huber, fault=None):
    """of the live edges given: residuals (E, 7), s^2, the cost, rho, and A, t_E for the Jacobians"""
    i, j = e[:, 0], e[:, 1]
    Mi, ti = sim_inv(M[i], t[i])
    MA, tA = sim_mul(M[j], t[j], Mi, ti)
    if fault == "z_inverted":
        ME, tE = sim_mul(MA, tA, Zm, Zt)
    else:
        Mz, tz = sim_inv(Zm, Zt)
        ME, tE = sim_mul(MA, tA, Mz, tz)
    with np.errstate(all="ignore"):
        cE = np.cbrt(det3(ME))
        r = np.concatenate([tE, log_so3(ME / cE[:, None, None]), np.log(cE)[:, None]], 1)
        s2 = w3[:, 0] * (r[:, :3] ** 2).sum(1) + w3[:, 1] * (r[:, 3:6] ** 2).sum(1) + w3[:, 2] * r[:, 6] ** 2
        s = np.sqrt(s2)
        rho, val = np.ones(len(e)), s2.copy()
        if huber > 0:
            over = s > huber
            rho[over] = huber / s[over]
            val[over] = huber * (2.0 * s[over] - huber)
    if fault == "no_irls":
        rho = np.ones(len(e))
    return dict(r=r, s2=s2, val=val, rho=rho, MA=MA, tA=tA, tE=tE)


def ldlt_solve(H, b):
    """natural-order LDL^T; None when a pivot is not > 0"""
    n = len(b)
    L, D = np.eye(n), np.zeros(n)
    for j in range(n):
        d = H[j, j] - sum(L[j, m] * L[j, m] * D[m] for m in range(j))
        if not d > 0:
            return None
        D[j] = d
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - sum(L[i, m] * L[j, m] * D[m] for m in range(j))) / d
    y = np.linalg.solve(L, b)
    x = np.linalg.solve(L.T, y / D)
    return x if np.all(np.isfinite(x)) else None


def run(S, edges, Z, weights=None, fixed=None, n_rounds=8, n_cg=8, cg_tol=1e-6, lambda0=1e-4, huber=0.0, with_scale=True,
        preconditioner="CHAIN", fault=None, reverse=False, solver="pcg"):
    """Returns a dict: S_out (F, 4, 4) float32 as the call leaves it, state (M, t) in double before the rounding, status, stats,
    rounds (dicts), edge_status, edge_cost, kind (per frame), H (F, 7, 7) undamped blocks at the final state, margins (how close
    every decision came: accept: |candidate - current| / current, stop: |r| / (cg_tol |r_0|))."""
    S32 = np.asarray(S, np.float32).reshape(-1, 4, 4)
    F = len(S32)
    M, t = mats(S32)
    cg_tol, lambda0, huber = float(np.float32(cg_tol)), float(np.float32(lambda0)), float(np.float32(huber))
    e_all, w_all, ok = live_edges(F, edges, weights)
    E = len(e_all)
    Zall = np.asarray(Z, np.float32).astype(np.float64).reshape(E, 4, 4) if E else np.zeros((0, 4, 4))
    live = np.nonzero(ok)[0]
    e, w3 = e_all[live], w_all[live]
    Zm, Zt = Zall[live][:, :3, :3], Zall[live][:, :3, 3]
    held = np.zeros(F, bool) if fixed is None else np.asarray(fixed).astype(bool)
    touched = np.zeros(F, bool)
    touched[e.ravel()] = True
    kind = np.where(held, HELD, np.where(touched, ACTIVE, ISOLATED))
    active = kind == ACTIVE
    mask = np.zeros((F, 7), bool)
    mask[active] = True
    if not with_scale:
        mask[:, 6] = False
    order = slice(None, None, -1) if reverse else slice(None)

    def total(ev):
        vals = np.zeros(E)
        vals[live] = ev["val"]
        return tree_sum(vals[order]) if reverse else tree_sum(vals)

    ev = evaluate(M, t, e, Zm, Zt, w3, huber, fault)
    cost_start = total(ev)
    s2_start = ev["s2"].copy()
    out = dict(kind=kind, edge_status=np.where(ok, EDGE_OK, EDGE_SKIPPED).astype(np.int32), rounds=[], margins=dict(accept=[], stop=[]))
    stats = dict(n_frames=F, n_edges=E, n_live_edges=len(live), n_free_frames=int((~held).sum()), n_active_frames=int(active.sum()),
                 n_accepted=0, cost_before=cost_start, cost_after=cost_start)
    status = (1 if not np.isfinite(cost_start) else 2 if not (~held).any() else 3 if len(live) == 0 else 2 if not active.any() else 0)

    def blocks(M, t, ev):
        """J_i, J_j (E, 7, 7), the weights (E, 7), g (F, 7), H_ff (F, 7, 7), the chain's W (F, 3)"""
        A, _ = ad_matrices(ev["MA"], ev["tA"])
        G = g_matrix(ev["tE"], fault)
        Ji = G @ A if fault == "ad_sign" else -(G @ A)
        Jj = G
        w7 = ev["rho"][:, None] * np.repeat(w3, [3, 3, 1], axis=1)
        g, H, wl, wa = np.zeros((F, 7)), np.zeros((F, 7, 7)), np.zeros((F, 3)), np.zeros((F, 3))
        # ascending 2 e + side: edge by edge, side 0 (the frame is i) before side 1
        idx = np.stack([e[:, 0], e[:, 1]], 1).ravel()
        J2 = np.stack([Ji, Jj], 1).reshape(-1, 7, 7)
        w2 = np.repeat(w7, 2, axis=0)
        r2 = np.repeat(ev["r"], 2, axis=0)
        other = np.stack([e[:, 1], e[:, 0]], 1).ravel()
        gt = np.einsum("kab,ka->kb", J2, w2 * r2)
        Ht = np.einsum("kab,ka,kac->kbc", J2, w2, J2)
        np.add.at(g, idx[order], gt[order])
        np.add.at(H, idx[order], Ht[order])
        np.add.at(wa, idx[order], w2[:, [0, 3, 6]][order])
        link = other == idx - 1
        np.add.at(wl, idx[link][order], w2[link][:, [0, 3, 6]][order])
        W = np.where(wl > 0, wl, np.where(wa > 0, wa, 1.0))
        return Ji, Jj, w7, g, H, W

    def h_times(p, Ji, Jj, w7, H, lam):
        y = w7 * (np.einsum("eab,eb->ea", Ji, p[e[:, 0]]) + np.einsum("eab,eb->ea", Jj, p[e[:, 1]]))
        idx = np.stack([e[:, 0], e[:, 1]], 1).ravel()
        c2 = np.stack([np.einsum("eab,ea->eb", Ji, y), np.einsum("eab,ea->eb", Jj, y)], 1).reshape(-1, 7)
        q = np.zeros((F, 7))
        np.add.at(q, idx[order], c2[order])
        if fault != "no_damping":
            q = q + lam * np.einsum("faa->fa", H) * p
        return np.where(mask, q, 0.0)

    def precondition(r, H, W, lam, M, t):
        """z = M^-1 r, or None when a pivot of JACOBI is not > 0"""
        z = np.zeros((F, 7))
        n = 7 if with_scale else 6
        if preconditioner == "JACOBI":
            for f in np.nonzero(active)[0]:
                D = H[f][:n, :n] + lam * np.diag(np.diag(H[f])[:n])
                x = ldlt_solve(D, r[f][:n])
                if x is None:
                    return None
                z[f, :n] = x
            return z
        A, Ai = ad_matrices(M, t)
        a = np.where(active[:, None], np.einsum("fab,fa->fb", A, r), 0.0)
        b, run_ = np.zeros((F, 7)), np.zeros(7)
        for f in range(F - 1, -1, -1):
            if not active[f] and fault != "chain_no_restart":
                run_ = np.zeros(7)
            if active[f]:
                run_ = run_ + a[f]
                b[f] = run_
        Wm = (1.0 + lam) * np.repeat(W, [3, 3, 1], axis=1)
        d = np.einsum("fab,fb->fa", Ai, np.einsum("fab,fa->fb", Ai, b) / Wm)
        d = np.where(active[:, None], d, 0.0)
        h, run_ = np.zeros((F, 7)), np.zeros(7)
        for f in range(F):
            if not active[f] and fault != "chain_no_restart":
                run_ = np.zeros(7)
            if active[f]:
                run_ = run_ + d[f]
                h[f] = run_
        z = np.einsum("fab,fb->fa", A, h)
        return np.where(mask, z, 0.0)

    H_last = np.zeros((F, 7, 7))
    if status != 0:
        out.update(S_out=S32.copy(), state=(M, t), status=status, stats=dict(stats, status=status), edge_cost=_edge_cost(E, live, s2_start), H=H_last,
                   rounds=[dict(cost=0.0, cost_candidate=0.0, lam=0.0, residual=0.0, cg_iterations=0, accepted=0)] * int(n_rounds))
        return out
    lam, cur, n_acc = lambda0, cost_start, 0
    for _ in range(int(n_rounds)):
        ev = evaluate(M, t, e, Zm, Zt, w3, huber, fault)
        Ji, Jj, w7, g, H, W = blocks(M, t, ev)
        H_last = H
        r = np.where(mask, -g, 0.0)
        x = np.zeros((F, 7))
        bad = nostep = False
        iters, rr0, rr = 0, float((r * r).sum()), float((r * r).sum())
        if solver == "dense":
            Hd = np.zeros((7 * F, 7 * F))
            for k in range(len(e)):
                a_, b_ = e[k]
                Jrow = np.zeros((7, 7 * F))
                Jrow[:, 7 * a_:7 * a_ + 7], Jrow[:, 7 * b_:7 * b_ + 7] = Ji[k], Jj[k]
                Hd += Jrow.T @ (w7[k][:, None] * Jrow)
            Hd += lam * np.diag(np.diag(Hd))
            m = mask.ravel()
            sol = np.zeros(7 * F)
            sol[m] = np.linalg.solve(Hd[np.ix_(m, m)], r.ravel()[m])
            x = sol.reshape(F, 7)
        else:
            z = precondition(r, H, W, lam, M, t)
            if z is None:
                bad = True
            else:
                p, rz = z.copy(), float((r * z).sum())
                for _k in range(int(n_cg)):
                    q = h_times(p, Ji, Jj, w7, H, lam)
                    pq = float((p * q).sum())
                    if not (pq > 0 and np.isfinite(pq)):
                        nostep = iters == 0
                        break
                    alpha = rz / pq
                    x = x + alpha * p
                    r = r - alpha * q
                    z = precondition(r, H, W, lam, M, t)
                    if z is None:
                        z = np.zeros((F, 7))
                    rz_new, rr = float((r * z).sum()), float((r * r).sum())
                    p = z + (rz_new / rz) * p
                    rz = rz_new
                    iters += 1
                    if cg_tol > 0 and rr0 > 0:
                        out["margins"]["stop"].append(np.sqrt(rr) / (cg_tol * np.sqrt(rr0)))
                    if not (np.sqrt(rr) > cg_tol * np.sqrt(rr0)):
                        break
        formed = not bad and not nostep
        cand, accept = 0.0, False
        if formed:
            Mc, tc = M.copy(), t.copy()
            for f in np.nonzero(active)[0]:
                Mc[f], tc[f] = apply_update(M[f], t[f], x[f], with_scale, fault)
            cand = total(evaluate(Mc, tc, e, Zm, Zt, w3, huber, fault))
            accept = bool(np.isfinite(cand) and cand <= cur) or fault == "accept_always"
            if cur > 0 and np.isfinite(cand):
                out["margins"]["accept"].append(abs(cand - cur) / cur)
        out["rounds"].append(dict(cost=cur, cost_candidate=cand if formed else 0.0, lam=lam,
                                  residual=(np.sqrt(rr / rr0) if rr0 > 0 else 0.0) if not bad else 0.0, cg_iterations=iters, accepted=int(accept)))
        if accept:
            M, t, cur, n_acc = Mc, tc, cand, n_acc + 1
            if fault == "round_every_round":
                M, t = M.astype(np.float32).astype(np.float64), t.astype(np.float32).astype(np.float64)
            if lam > 0:
                lam = max(lam / 10.0, 1e-12)
        else:
            lam = max(10.0 * lam, 1e-6)
    Mr, tr = M.astype(np.float32).astype(np.float64), t.astype(np.float32).astype(np.float64)
    ev_end = evaluate(Mr, tr, e, Zm, Zt, w3, huber, fault)
    final = total(ev_end)
    if n_rounds > 0 and n_acc == 0:
        status = 4
    elif not final <= cost_start:
        status = 5
    write = status == 0 and n_acc > 0
    S_out = S32.copy()
    if write:
        for f in np.nonzero(active)[0]:
            S_out[f] = np.eye(4, dtype=np.float32)
            S_out[f, :3, :3], S_out[f, :3, 3] = Mr[f], tr[f]
    if n_rounds == 0 or n_acc == 0:
        ev0 = evaluate(M, t, e, Zm, Zt, w3, huber, fault)
        H_last = blocks(M, t, ev0)[4]
    out.update(S_out=S_out, state=(M, t), status=status, H=H_last,
               stats=dict(stats, status=status, n_accepted=n_acc, cost_after=final),
               edge_cost=_edge_cost(E, live, ev_end["s2"] if write else s2_start))
    return out


def _edge_cost(E, live, s2):
    c = np.zeros(E)
    c[live] = s2
    return c


# ---- the measure of the GPU test ----
def step_between(S_from, S_to):
    """the left perturbation (tau, omega, sigma) that takes the similarity S_from (M, t in double) to S_to, to first order:
    E = S_to S_from^-1, d = (t_E, log R_E, ln c_E)"""
    Mi, ti = sim_inv(S_from[0], S_from[1])
    ME, tE = sim_mul(S_to[0], S_to[1], Mi, ti)
    cE = np.cbrt(det3(ME))
    return np.concatenate([tE, log_so3(ME / cE[..., None, None]), np.log(cE)[..., None]], -1)


def distance(ref, S_kept):
    """per frame sqrt(d^T H_ff d) from the restatement's double state to a stored float32 state (F, 4, 4), in the blocks of the
    restatement's final state: the cost's own unit"""
    Ms, ts = mats(S_kept)
    d = step_between(ref["state"], (Ms, ts))
    return np.sqrt(np.maximum(np.einsum("fa,fab,fb->f", d, ref["H"], d), 0.0))


def half_ulp(ref, S_kept):
    """half an ulp of each of the 12 stored entries of every frame, turned into a bound of the 7-vector (dS S^-1: tau <= |dt| +
    |dM M^-1| |t|, omega and sigma <= the entries of |dM| |M^-1|) and carried through |H_ff|"""
    S = np.asarray(S_kept, np.float32).reshape(-1, 4, 4)
    u = (np.spacing(np.abs(S)).astype(np.float64) / 2.0)
    Ms, ts = mats(S)
    B = u[:, :3, :3] @ np.abs(inv3(Ms))
    tau = u[:, :3, 3] + np.einsum("fij,fj->fi", B, np.abs(ts))
    om = np.stack([(B[:, 2, 1] + B[:, 1, 2]) / 2, (B[:, 0, 2] + B[:, 2, 0]) / 2, (B[:, 1, 0] + B[:, 0, 1]) / 2], 1)
    sg = (B[:, 0, 0] + B[:, 1, 1] + B[:, 2, 2]) / 3
    d = np.concatenate([tau, om, sg[:, None]], 1)
    return np.sqrt(np.einsum("fa,fab,fb->f", d, np.abs(ref["H"]), d))
