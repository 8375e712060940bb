"""f64 CPU restatements of the refit kernels (dr_refit_fundamental, dr_refit_essential) and the inputs their tests share.
No device code.  Written from oracle/cpu_ref.py: the F refit is `fundamental_8pt` on the selected rows with the null vector
taken two independent ways, the E refit is `nister_5pt` on the selected rows as one sample.

The F restatement is its own yardstick: the smallest eigenvector of the 9x9 Gram matrix A^T A (torch.linalg.eigh) and the
last right singular vector of the design matrix A (torch.linalg.svd) are the same vector, and how far the two computed
ones are apart bounds what either is worth.  Perturbation theory puts that distance at a small multiple of
eps64 * cond with cond = lambda_1 / (lambda_8 - lambda_9); REF_AGREEMENT is the multiple measured on every input below
(tests/test_refit_ref.py recomputes it), and the device tolerance is ten times that (f_tolerance)."""
import torch

from differentiable_ransac_amd import synth
from oracle import cpu_ref as O

EPS64 = float(torch.finfo(torch.float64).eps)
EPS32 = float(torch.finfo(torch.float32).eps)

# worst  distance(eigh form, svd form) / (eps64 * cond)  over all_f_inputs() -- every F input of tests/test_gpu_refit.py, f64 and
# rounded to f32, unweighted and weighted.  Measured 13.4 (the constant is its ceiling); test_refit_ref.py fails if an input
# exceeds it.
REF_AGREEMENT = 14.0
F_TOL_FLOOR = 1e-11

RATIO_BINS = ((0.0, 0.1), (0.5, 0.7), (0.7, 0.9), (0.9, 0.97))   # the last one is closed: [0.9, 0.97]
MIN_PER_BIN = 8
MAX_COND = 1e4


def rel_err(F, Fref):
    """|F - Fref|_max / |Fref|_max after sign alignment (the metric of test_batched_refit_kernels)"""
    F, Fref = F.double(), Fref.double()
    s = torch.sign((F * Fref).sum())
    return float((F * s - Fref).abs().max() / Fref.abs().max())


def f_tolerance(cond, dtype):
    """bound on rel_err(kernel, f_refit): ten times what the two references differ by, floored; plus the rounding of an f32 output"""
    tol = max(F_TOL_FLOOR, 10.0 * REF_AGREEMENT * EPS64 * cond)
    return tol + (8 * EPS32 if dtype == torch.float32 else 0.0)


def f_refit_forms(matches, mask=None, weights=None):
    """Both forms of the F refit of one pair.  -> dict(F_svd, F_eigh, valid, cond, ratio, distance, lam [9] ascending)"""
    m = matches.double()
    sel = m if mask is None else m[mask.bool()]
    w = None if weights is None else (weights.double() if mask is None else weights.double()[mask.bool()])
    if sel.shape[0] < 8:
        eye = torch.eye(3, dtype=torch.float64)
        return dict(F_svd=eye, F_eigh=eye.clone(), valid=False, cond=float("nan"), ratio=float("nan"), distance=0.0, lam=None)
    n, T1, T2t = O.hartley_normalize(sel[None])          # unweighted normalisation of the selected rows
    A = O._f_rows(n, None if w is None else w[None])[0]  # weights scale the rows
    lam, vec = torch.linalg.eigh(A.T @ A)                # ascending
    _, _, vh = torch.linalg.svd(A, full_matrices=True)   # (8 rows: the ninth right singular vector is the exact null vector)
    back = lambda f: (T2t[0] @ f.reshape(3, 3) @ T1[0])
    F_svd, F_eigh = back(vh[-1]), back(vec[:, 0])
    lam9, lam8, lam1 = float(lam[0]), float(lam[1]), float(lam[-1])
    return dict(F_svd=F_svd, F_eigh=F_eigh, valid=True, cond=lam1 / (lam8 - lam9), ratio=max(lam9, 0.0) / lam8,
                distance=rel_err(F_eigh, F_svd), lam=lam)


def f_refit(matches, mask=None, weights=None):
    """matches [N,4], mask [N] bool | None, weights [N] | None -> (F [3,3] f64, valid, cond, ratio): the SVD form.
    Below 8 selected rows: the identity and valid = False, as the kernel documents (cond, ratio = nan)."""
    r = f_refit_forms(matches, mask, weights)
    return r["F_svd"], r["valid"], r["cond"], r["ratio"]


def e_refit(matches, mask=None):
    """five-point solver on the selected rows as ONE sample -> (E [10,3,3] f64, real [10]); compare as solution sets"""
    m = matches.double()
    sel = m if mask is None else m[mask.bool()]
    E, ok, real = O.nister_5pt(sel[None])
    return E[0], real[0] & ok[0]


def set_distance(E, valid, Eo, valid_o):
    """worst distance of the two solution sets, both directions, and the two counts"""
    E, Eo = E.cpu().double(), Eo.cpu().double()
    valid, valid_o = valid.cpu().bool(), valid_o.cpu().bool()
    fw = O.match_solution_sets(E, valid, Eo, valid_o)
    bw = O.match_solution_sets(Eo, valid_o, E, valid)
    worst = max([0.0] + [float(x) for x in fw] + [float(x) for x in bw])
    return worst, int(valid.sum()), int(valid_o.sum())


# ------------------------------------------------------------------------------------------------------------ inputs
_PAIRS = {}


def _pair(seed, pixel):
    key = (int(seed), bool(pixel))
    if key not in _PAIRS:   # 2000 rows: [0, 1000) outliers, [1000, 2000) inliers, noise 1e-3
        _PAIRS[key] = synth.two_view_pair(seed, 2000, pixel=pixel, noise=1e-3, dtype=torch.float64)
    return _PAIRS[key]


def contaminated(seed, n_in, n_out, N, pixel=True):
    """n_in inliers + n_out outliers of synthetic pair `seed`, selected, at seeded positions of an N-row pair; the other rows are
    unselected filler (further rows of the same pair).  -> matches [N,4] f64, mask [N] bool"""
    assert n_in + n_out <= N <= 2000 - n_in - n_out and max(n_in, n_out) <= 1000
    m = _pair(seed, pixel)["matches"]
    g = torch.Generator().manual_seed(1000003 * int(seed) + 1009 * n_in + n_out)
    pos = torch.randperm(N, generator=g)[: n_in + n_out]
    rest = torch.cat((m[n_out:1000], m[1000 + n_in:]))
    out = rest[torch.randperm(rest.shape[0], generator=g)[:N]].clone()
    out[pos] = torch.cat((m[1000:1000 + n_in], m[:n_out]))
    mask = torch.zeros(N, dtype=torch.bool)
    mask[pos] = True
    return out, mask


# the eigen-gap sweep: (n_in, n_out) x seeds, every selection at most 64 rows of a 320-row pair (two strides of the block, the second
# one partial).  Chosen by ratio and cond of the f64 Gram matrix alone (test_refit_ref.py holds the coverage condition).
SWEEP_N = 320
SWEEP_FAMILIES = ((64, 0), (16, 16), (32, 32), (20, 20), (12, 12), (28, 36), (10, 6), (12, 4))
SWEEP_SEEDS = ((0, 1, 2, 3, 4, 5, 6, 7, 8, 9),                  # ratio < 0.03
               (1, 2, 7, 9, 14, 16, 18, 25, 26, 38, 21),        # ten in [0.5, 0.7), seed 21: 0.96
               (6, 7, 11, 13, 14, 15, 16, 25, 34, 40, 28),      # ten in [0.7, 0.9), seed 28: 0.91
               (11, 15),                                        # 0.95, 0.91
               (12, 15),                                        # 0.93, 0.93
               (40, 43, 46, 49),                                # 0.91 ... 0.94
               (7, 14, 15),                                     # 0.72 ... 0.77 on 16 rows
               (6, 13, 14, 18))                                 # 0.3 ... 0.4: between the bins


def sweep_cases():
    """[(label, matches [N,4], mask [N])]: at most 64, one launch"""
    out = []
    for (a, b), seeds in zip(SWEEP_FAMILIES, SWEEP_SEEDS):
        for s in seeds:
            m, k = contaminated(s, a, b, SWEEP_N)
            out.append((f"{a}+{b}/s{s}", m, k))
    return out


def moderate_weights(n_cases, N, seed=5):
    """row weights 0.2 + 0.8 u, [n_cases, N]"""
    return 0.2 + 0.8 * torch.rand(n_cases, N, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def wide_weights(N, seed=6):
    """row weights spanning 1e-5 ... 1, log-uniform, [N]"""
    u = torch.rand(N, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    w = 10.0 ** (-5.0 * u)
    w[0], w[1] = 1.0, 1e-5
    return w


def wide_weight_case():
    """clean inliers (a wide gap stays a well-posed problem under weights of five decades) -> matches, mask, weights"""
    m, k = contaminated(3, 64, 0, SWEEP_N)
    return m, k, wide_weights(SWEEP_N)


# ---- point-count and layout edges
EDGE_NS = (9, 63, 64, 65, 255, 256, 257, 511, 513, 1000)   # plus the minimal count in front: 8 (F) / 5 (E)
LAYOUT_N = 1000


def clean_pair(seed, N, pixel, noise=True):
    """N inlier rows of a synthetic pair (noise 1e-3, or noise-free with gt) -> matches [N,4] f64, gt model"""
    if noise:
        d = _pair(seed, pixel)
        return d["matches"][1000:1000 + N].clone(), (d["gt_F"] if pixel else d["gt_E"])
    d = synth.two_view_pair(seed, 2 * N, pixel=pixel, noise=0.0, dtype=torch.float64)
    return d["matches"][N:].clone(), (d["gt_F"] if pixel else d["gt_E"])


def layout_masks(kmin):
    """{name: mask [1000]} for kmin = 8 (F) / 5 (E) rows the solve needs"""
    N = LAYOUT_N
    idx = torch.arange(N)
    g = torch.Generator().manual_seed(77)
    scattered = torch.randperm(N, generator=g)
    def of(ix):
        k = torch.zeros(N, dtype=torch.bool)
        k[ix] = True
        return k
    return {
        "one_thread": idx % 256 == 0,              # 4 rows: one thread of the block, and below either minimum
        "first_wave": of(scattered[scattered < 64][:40]),
        "last_wave_first_stride": (idx >= 192) & (idx < 256),
        "last_rows": idx >= N - kmin,
        "exactly_min": of(scattered[:kmin]),
        "min_plus_one": of(scattered[:kmin + 1]),
        "below_min": of(scattered[:kmin - 1]),
        "none": torch.zeros(N, dtype=torch.bool),
    }


ONE_THREAD_LONG_N = 256 * 9 + 1   # ten rows at indices = 0 (mod 256): a whole selection in one thread, above both minima


def all_f_inputs():
    """every (label, matches, mask, weights) the GPU tests hand the F kernel and compare with f_refit, f64 values"""
    out = [(lab, m, k, None) for lab, m, k in sweep_cases()]
    w = moderate_weights(len(out), SWEEP_N)
    out += [("w:" + lab, m, k, w[i]) for i, (lab, m, k, _) in enumerate(list(out))]
    out.append(("wide_weights",) + wide_weight_case())
    for N in (8,) + EDGE_NS:
        out.append((f"N={N}", clean_pair(11, N, True)[0], None, None))
    m = clean_pair(12, LAYOUT_N, True)[0]
    for name, k in layout_masks(8).items():
        if int(k.sum()) >= 8:
            out.append(("layout:" + name, m, k, None))
    mk = torch.arange(ONE_THREAD_LONG_N) % 256 == 0
    out.append(("one_thread_long", long_pair(), mk, None))
    return out


def long_pair(pixel=True):
    d = synth.two_view_pair(13, 2 * ONE_THREAD_LONG_N, pixel=pixel, noise=1e-3, dtype=torch.float64)
    return d["matches"][ONE_THREAD_LONG_N:].clone()


def long_pair_normalised():
    return long_pair(False)


E_FORM_N = 257


def e_form_cases():
    """16 x (label, matches [257,4] in normalised coordinates, mask): eight clean pairs (all rows) and eight selections of
    40 inliers + 24 outliers, whose Gram matrix has its small eigenvalues close together"""
    out = [(f"clean/s{s}", clean_pair(s, E_FORM_N, False)[0], torch.ones(E_FORM_N, dtype=torch.bool)) for s in range(30, 38)]
    for s in range(30, 38):
        m, k = contaminated(s, 40, 24, E_FORM_N, pixel=False)
        out.append((f"40+24/s{s}", m, k))
    return out


def poor_model(gt, seed):
    """the ground truth with every entry off by about a half: a model almost nothing agrees with"""
    g = torch.Generator().manual_seed(int(seed))
    return gt.double() * (1 + 0.5 * torch.randn(3, 3, generator=g, dtype=torch.float64))


def lo_bad_start(seed, N=256, frac_in=0.6, pixel=True):
    """a pair of N rows and a state mask of 60 % inliers + 40 % outliers at seeded positions -> matches [N,4] f64, mask [N],
    K1, K2, gt"""
    d = _pair(seed, pixel)
    n_sel = N // 2
    n_in = int(round(frac_in * n_sel))
    m, k = contaminated(seed, n_in, n_sel - n_in, N, pixel)
    return m, k, d["K1"], d["K2"], (d["gt_F"] if pixel else d["gt_E"])
