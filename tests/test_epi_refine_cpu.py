"""The refit of vo_refine_transform as include/vo_hip.h states it, in float64 numpy (tests/epi_refine_restatement.py): the
analytic Jacobian against central differences, the gain over the linear 8-point fit on noisy frame pairs, the accept rule
and the noise-free example data.  No GPU: the linear fit is the oracle-side one."""
import os

import numpy as np
import pytest

import epi_refine_restatement as E
from oracle import vo_pipeline as vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "example_data", "data")


def _random_problem(vo, rng, n=50):
    X = vo.synth.random_isometry(rng, 1.0, 1.0).astype(np.float64)
    t = X[:3, 3]
    x1 = np.stack([rng.uniform(0, 639, n), rng.uniform(0, 479, n), np.ones(n)], axis=1)
    x2 = np.stack([rng.uniform(0, 639, n), rng.uniform(0, 479, n), np.ones(n)], axis=1)
    Kinv = np.linalg.inv(vo.synth.K_REF.astype(np.float64))
    return Kinv, X[:3, :3], t / np.linalg.norm(t), x1, x2


def _central(f, h=1e-6):
    cols = []
    for p in range(5):
        d = np.zeros(5)
        d[p] = h
        cols.append((f(d) - f(-d)) / (2 * h))
    return np.stack(cols, axis=-1)


@pytest.mark.parametrize("pose", range(5))
def test_jacobian_equals_central_differences(vo, pose):
    """50 random pairs under a random pose: d r / d(parameters), and -- with and without the Huber branch active -- the
    gradient J^T w r of the Huber loss sum(rho), rho = r^2/2 for |r| <= delta, delta (|r| - delta/2) beyond"""
    Kinv, R, th, x1, x2 = _random_problem(vo, np.random.default_rng(100 + pose))
    r, J, ok = E.jacobian(Kinv, R, th, x1, x2)
    assert ok.all()
    Jn = _central(lambda d: E.residuals(Kinv, *E.apply_step(R, th, d), x1, x2)[0])
    assert np.abs(J - Jn).max() <= 1e-6 * np.abs(J).max(), np.abs(J - Jn).max() / np.abs(J).max()
    for delta in (0.0, float(np.median(np.abs(r)))):            # none; half of the pairs on the linear branch

        def loss(d):
            rr = E.residuals(Kinv, *E.apply_step(R, th, d), x1, x2)[0]
            if not delta > 0:
                return np.sum(0.5 * rr * rr)
            a = np.abs(rr)
            return np.sum(np.where(a <= delta, 0.5 * rr * rr, delta * (a - 0.5 * delta)))

        w = E.huber_weights(r, delta)
        assert delta == 0.0 or 10 <= int((w < 1).sum()) <= 40
        g = J.T @ (w * r)
        gn = _central(loss)
        assert np.abs(g - gn).max() <= 1e-6 * np.abs(g).max(), (delta, np.abs(g - gn).max() / np.abs(g).max())


def test_basis_rule_and_step_keep_the_sphere():
    b1, b2 = E.tangent_basis(np.array([0.6, 0.0, 0.8]))
    assert np.allclose(b1, [-0.8, 0.0, 0.6]) and np.allclose(b2, np.cross([0.6, 0.0, 0.8], b1))      # k = 1
    s = 1.0 / np.sqrt(3.0)
    b1, _ = E.tangent_basis(np.array([s, -s, s]))                # a tie: the lowest axis, k = 0
    assert np.allclose(b1, np.cross([s, -s, s], [1, 0, 0]) / np.linalg.norm(np.cross([s, -s, s], [1, 0, 0])))
    R, th = E.apply_step(np.eye(3), np.array([0.0, 0.0, 1.0]), np.array([0.1, -0.2, 0.3, 0.05, -0.02]))
    assert abs(np.linalg.norm(th) - 1) < 1e-15 and np.abs(R @ R.T - np.eye(3)).max() < 1e-15


@pytest.fixture(scope="module")
def noisy_runs(vo, o32):
    """frame_pair(2000, seed = 2000 .. 2011, noise 0.5 px), true pairs: the linear fit and 10 plain rounds from it"""
    out = []
    for seed in range(2000, 2012):
        fp = vo.synth.frame_pair(2000, seed=seed, noise_px=0.5)
        X_lin = vp.estimate_transform(o32, fp["K"], fp["gt_matches"], fp["ref_pts"], fp["cur_pts"])
        X_ref, st = E.refine_transform(fp["K"], fp["gt_matches"], fp["ref_pts"], fp["cur_pts"], X_lin, 10, 0.0)
        out.append((fp, X_lin, X_ref, st))
    return out


def test_refit_beats_the_linear_fit(noisy_runs):
    lin = np.array([E.pose_errors(X_lin, fp["X_gt"]) for fp, X_lin, _, _ in noisy_runs])
    ref = np.array([E.pose_errors(X_ref, fp["X_gt"]) for fp, _, X_ref, _ in noisy_runs])
    print("median rotation error: linear %.3g refined %.3g; translation direction: linear %.3g refined %.3g; better in %d/12"
          % (np.median(lin[:, 0]), np.median(ref[:, 0]), np.median(lin[:, 1]), np.median(ref[:, 1]), (ref[:, 1] < lin[:, 1]).sum()))
    assert all(st["status"] == E.OK and st["rounds"] == 10 for _, _, _, st in noisy_runs)
    assert np.median(ref[:, 1]) <= 0.6 * np.median(lin[:, 1])
    assert np.median(ref[:, 0]) <= 0.8 * np.median(lin[:, 0])
    assert (ref[:, 1] < lin[:, 1]).sum() >= 9
    for _, X_lin, X_ref, st in noisy_runs:
        tn = np.linalg.norm(X_lin[:3, 3].astype(np.float64))
        assert abs(np.linalg.norm(X_ref[:3, 3]) - tn) <= 1e-12 * tn
        assert st["cost_after"] <= st["cost_before"] and st["n_used"] == 2000 and st["n_skipped"] == st["n_bad"] == 0


@pytest.mark.parametrize("seed", [2000, 2001, 2002, 2003])
@pytest.mark.parametrize("n_rounds", [1, 3, 10])
def test_accept_rule_from_a_start_half_a_radian_off(vo, noisy_runs, seed, n_rounds):
    fp, X_lin = noisy_runs[seed - 2000][:2]
    rng = np.random.default_rng(seed)
    X_bad = X_lin.copy()
    X_bad[:3, :3] = (vo.synth.rodrigues(rng.uniform(-1, 1, 3), 0.5) @ X_lin[:3, :3].astype(np.float64)).astype(np.float32)
    args = (fp["K"], fp["gt_matches"], fp["ref_pts"], fp["cur_pts"])
    X, st = E.refine_transform(*args, X_bad, n_rounds, 0.0)
    c_in, c_out = E.cost_of(*args[:1], X_bad, *args[1:]), E.cost_of(*args[:1], X, *args[1:])
    assert c_out <= c_in
    if st["status"] == E.OK:
        assert st["cost_after"] <= st["cost_before"] == c_in and abs(c_out - st["cost_after"]) <= 1e-9 * c_in
    else:
        assert st["status"] in (E.COST_ROSE, E.SINGULAR)
        assert X is X_bad or X.tobytes() == X_bad.tobytes()
        assert st["cost_after"] == st["cost_before"]


def test_statuses_of_the_restatement(noisy_runs):
    fp, X_lin = noisy_runs[0][:2]
    p, a, b = fp["gt_matches"], fp["ref_pts"], fp["cur_pts"]
    X, st = E.refine_transform(fp["K"], p[:7], a, b, X_lin)
    assert st["status"] == E.FEW_PAIRS and X is X_lin and st["n_used"] == 7 and st["rounds"] == 0
    wild = p.copy()
    wild[5, 1] = len(b)
    X, st = E.refine_transform(fp["K"], wild, a, b, X_lin)
    assert st["status"] == E.BAD_INDEX and st["n_bad"] == 1 and X is X_lin
    Z = X_lin.copy()
    Z[:3, 3] = 0
    X, st = E.refine_transform(fp["K"], p, a, b, Z)
    assert st["status"] == E.BAD_INPUT and X is Z and st["n_used"] == 0 and st["n_skipped"] == len(p)
    mask = np.arange(len(p)) % 2 == 0
    Xm, sm = E.refine_transform(fp["K"], p, a, b, X_lin, mask=mask)
    Xs, ss = E.refine_transform(fp["K"], p[mask], a, b, X_lin)
    assert sm["n_used"] == ss["n_used"] == 1000 and sm["n_skipped"] == 1000 and np.allclose(Xm, Xs, rtol=0, atol=1e-12)


def test_library_exports_the_refit_entry_points(vo):
    """no device needed: both entry points exist, the Python mirrors have the header's layout, the status words agree with
    the restatement's, and the header states what a caller must be able to restate"""
    import ctypes as C
    import re
    lib = vo.load_library()
    assert hasattr(lib, "vo_refine_transform") and hasattr(lib, "vo_refine_transform_dev")
    assert C.sizeof(vo.EpiRefineParams) == 8 and vo.EpiRefineParams.huber_px.offset == 4
    assert C.sizeof(vo.EpiRefineStats) == 40 and vo.EpiRefineStats.cost_before.offset == 24 and vo.EpiRefineStats.cost_after.offset == 32
    hdr = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    words = dict(re.findall(r"#define VO_EPI_REFINE_([A-Z_]+)\s+(\d+)", hdr))
    assert {k: int(v) for k, v in words.items()} == {name: code for code, name in E.STATUS_NAMES.items()}
    assert tuple(E.STATUS_NAMES[i] for i in range(6)) == vo.EPI_REFINE_STATUS
    for text in ("typedef struct vo_epi_refine_params", "typedef struct vo_epi_refine_stats", "K^-T R^T [th]x^T K^-1", "smallest |th_k|",
                 "X_in bit for bit", "1e-12", "Precedence: BAD_INDEX"):
        assert text in hdr, text
    assert lib.vo_abi_version() == 1


def test_noise_free_example_data_stays_put(o32):
    r = vp.run_real_init(DATA, o32)
    X, st = E.refine_transform(r["K"], r["corr"], r["p0"], r["p1"], r["X"], 10, 0.0)
    d = float(np.abs(np.asarray(X, np.float64) - r["X"].astype(np.float64)).max())
    print("example data: status %s, cost %.3g -> %.3g, max |refined - linear| = %.3g" % (E.STATUS_NAMES[st["status"]], st["cost_before"], st["cost_after"], d))
    assert d <= 1e-5
