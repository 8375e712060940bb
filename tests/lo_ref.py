"""f64 CPU restatement of test-mode RANSAC with local optimisation (RANSAC.__call__ + localOptimization, ransac.py:55-257,
lo = 1 / 2), built from the oracle's functions.  It is the arbiter of the device kernel (dr_local_opt) and of the drivers
that call it, as oracle.cpu_ref.ransac_test is for lo = 0.

The local-optimisation step follows the decided deviations of DESIGN.md section 5: the essential refit is the five-point
solver on the inlier rows in f64 and only its real solutions compete; with fewer than 8 (F) / 5 (E) inliers the pair is
left unchanged; the loop also stops when an accepted refit leaves the mask unchanged (exact: the next refit would see the
same rows)."""
import torch

from oracle import cpu_ref as O


def lo_step(matches, thr, fmat, lo, lo_iters, best_score, best_mask, best_model):
    """localOptimization (ransac.py:220-257) on one pair.  Returns (score, mask, model, refits run)."""
    refits = 0
    for _ in range(1 if lo == 1 else lo_iters):
        inl = best_mask.nonzero(as_tuple=True)[0]
        if inl.numel() < (8 if fmat else 5):
            break
        pts = matches[inl].unsqueeze(0).double()
        if fmat:
            cand = O.fundamental_8pt(pts)
            ok = torch.ones(1, dtype=torch.bool)
        else:
            E, sample_ok, real = O.nister_5pt(pts)
            cand, ok = E[0], real[0] & sample_ok[0]
        refits += 1
        cand = cand.to(matches.dtype)
        ok = ok & torch.isfinite(cand).flatten(1).all(-1)
        if not bool(ok.any()):
            break
        scores, masks = O.msac_score(matches, cand, thr)
        scores = torch.where(ok & ~torch.isnan(scores), scores, torch.full_like(scores, -float("inf")))
        b = int(torch.argmax(scores))
        if not float(scores[b]) >= best_score:                   # ransac.py:252: a tie is taken
            break
        changed = bool((masks[b] != best_mask).any())
        best_score, best_mask, best_model = float(scores[b]), masks[b], cand[b]
        if not changed:
            break
    return best_score, best_mask, best_model, refits


def ransac_test_lo(matches, logits, gumbel_batches, K1, K2, solver: str, lo: int, lo_iters: int = 64,
                   threshold: float = 0.75, max_iterations: int = 5000, confidence: float = 0.999, tau: float = 1.0,
                   refit: bool = True, num_samples=None, sample_size=None):
    """oracle.cpu_ref.ransac_test (lo = 0) with the local optimisation after every new best model.
    sample_size: the exponent of the adaptive stop; None = the estimator's sample_size, as in the reference, oracle.cpu_ref.ransac_test
    and the device drivers: 7 for the 8-point F estimator, 5 for the five-point one, whatever num_samples is.
    Returns best_model [3,3], best_mask [N], best_score, iterations, refits (total LSQ refits of the local optimisation)."""
    fmat = solver == "f8"
    k = num_samples or (8 if fmat else 5)
    ks = sample_size or (7 if fmat else 5)
    thr = O.normalized_threshold(threshold, K1, K2, fmat)
    N = matches.shape[0]
    it, best_score, best_mask, best_model = 0, 0.0, None, None
    max_iters = max_iterations
    refits = 0
    for g in gumbel_batches:
        if it >= max_iters:
            break
        B = g.shape[0]
        idx, ret, _ = O.gumbel_topk(logits, g, tau, k)
        samples = O.gather_samples(matches, ret)
        if fmat:
            models = O.fundamental_8pt(samples)
        else:
            E, ok, _ = O.nister_5pt(samples)
            models = O.compact_models(E, ok)
        scores, masks = O.msac_score(matches, models, thr)
        b = int(torch.argmax(scores))
        if float(scores[b]) > best_score or it == 0:
            best_score, best_mask, best_model = float(scores[b]), masks[b], models[b]
            if lo:
                best_score, best_mask, best_model, n = lo_step(matches, thr, fmat, lo, lo_iters, best_score, best_mask,
                                                               best_model)
                refits += n
            max_iters = min(max_iterations, O.adaptive_iteration_number(int(best_mask.sum()), N, ks, confidence,
                                                                        max_iterations=max_iterations))
        it += B
    if refit:
        inl = best_mask.nonzero(as_tuple=True)[0]
        if fmat:
            cand = O.fundamental_8pt(matches[inl].unsqueeze(0))
        else:
            E, ok, _ = O.nister_5pt(matches.unsqueeze(0).double())
            cand = O.compact_models(E, ok).to(matches.dtype)
        scores, _ = O.msac_score(matches, cand, thr)
        if float(scores.max()) > best_score:
            b = int(torch.argmax(scores))
            best_model, best_score = cand[b], float(scores[b])
    return best_model, best_mask, best_score, it, refits
