"""The training losses that follow the hot path: MatchLoss and PoseLoss for the two-view drivers,
RegistrationLoss for the 3-D registration driver, HomographyLoss for the homography driver (with the evaluation metrics
registration_errors and homography_errors) and, at the end, PnPLoss and PnPExpectedLoss (DSAC) for the absolute-pose driver and
RegistrationExpectedLoss and HomographyExpectedLoss, the same expected loss on the registration and the homography drivers'
hypotheses.

MatchLoss -- the clamped symmetric-epipolar training loss of the reference (loss.py:107-153), on the fused kernel
`dr_episym_fwd/bwd`.

The reference obtains the ground-truth inlier mask from `cv2.recoverPose(gt_E, pts1, pts2)` (cheirality of the
triangulated points, loss.py:99,134).  Pass either the mask (`gt_mask [P,N] bool`) or the ground-truth essential matrices
(`gt_E [P,3,3]`: the mask is then computed by `ops.recover_pose_mask`, the same Horn decomposition + cheirality vote as
the pose-error kernel); neither = all points.  Everything else follows the reference: per pair, mean over (models x
masked points) of min(error, 1); then the mean over pairs."""
import torch

from . import ops


def calibrate(models, pts1, pts2, K1, K2, im_size1, im_size2):
    """The F branch shared by the three losses (loss.py:36-49,81-92,118-121): E = K2^T F K1 and the points mapped from
    image-size-normalised to calibrated coordinates -- normalize_keypoints_tensor(denormalize_pts(pts, im_size), K)
    (cv_utils.py:35-45, feature_utils.py:40-49).  models [P,M,3,3], pts [P,N,2], K [P,3,3], im_size [P,2] = (h, w)."""
    Es = K2.transpose(-1, -2)[:, None] @ models @ K1[:, None]

    def to_camera(pts, K, im_size):
        scale = im_size.max(dim=-1).values[:, None, None]
        centre = torch.stack((im_size[:, 1] / 2, im_size[:, 0] / 2), dim=-1)[:, None, :]
        px = pts * scale + centre
        c = torch.stack((K[:, 0, 2], K[:, 1, 2]), dim=-1)[:, None, :]
        f = torch.stack((K[:, 0, 0], K[:, 1, 1]), dim=-1)[:, None, :]
        return (px - c) / f
    return Es, to_camera(pts1, K1, im_size1), to_camera(pts2, K2, im_size2)


class MatchLoss(object):
    def __init__(self, fmat=False):
        self.fmat = fmat

    def reference_forward(self, models, gt_E, pts1, pts2, K1=None, K2=None, im_size1=None, im_size2=None, topk_flag=False,
                          k=1, keep=None):
        """The reference's signature (loss.py:114): models [P,M,3,3] (F in the F branch), gt_E [P,3,3], pts [P,N,2].
        topk_flag: average only the k models with the smallest mean error per pair."""
        if self.fmat:
            models, pts1, pts2 = calibrate(models, pts1, pts2, K1, K2, im_size1, im_size2)
        matches = torch.cat((pts1, pts2), dim=-1).to(models.dtype).contiguous()
        if not topk_flag:
            return self.forward(models, matches, keep=keep, gt_E=gt_E.to(models.dtype))
        with torch.no_grad():
            gt_mask = ops.recover_pose_mask(matches, gt_E.to(models.dtype))[0][:, 0]
        sums = ops.episym_sums(matches, gt_mask, models, keep)
        per_model = sums / gt_mask.sum(1, keepdim=True).to(sums.dtype).clamp(min=1.0)
        if keep is not None:
            per_model = torch.where(keep, per_model, torch.full_like(per_model, float("inf")))
        return torch.topk(per_model, k=k, dim=1, largest=False).values.mean(1).mean()

    def forward(self, models, matches, gt_mask=None, keep=None, gt_E=None):
        """models [P,M,3,3] (E, or F already mapped to normalised coordinates), matches [P,N,4] normalised, gt_mask [P,N]
        or gt_E [P,3,3], keep [P,M] bool (models to average over; None = all) -> scalar loss."""
        if gt_mask is None and gt_E is not None:
            with torch.no_grad():
                gt_mask = ops.recover_pose_mask(matches, gt_E)[0][:, 0]
        # per pair: sum of the clamped errors / max(#masked points * #kept models, 1), then the mean over the pairs -- two
        # launches forward, one backward; one pass and one elementwise launch when the models require grad (ops.match_loss_mean)
        return ops.match_loss_mean(matches, gt_mask, models, keep)

    __call__ = forward


class PoseLoss(object):
    """PoseLoss (loss.py:11-68): per pair the mean over the pair's models of (err_R + err_t) / 2 in degrees, then the mean
    over pairs; `svd=False` (Horn decomposition, what train.py:82-93 passes; differentiable) or `svd=True` (decompose_E,
    forward only).  One launch (`dr_pose_error_fwd` / `dr_pose_error_svd_fwd`) instead of a Python loop over models with
    four cv2.triangulatePoints calls each."""

    def __init__(self, fmat=False):
        self.fmat = fmat

    def forward_average(self, estimated_models, pts1, pts2, gt_R, gt_t, K1=None, K2=None, im_size1=None, im_size2=None,
                        svd=False, keep=None):
        """estimated_models [P,M,3,3] (F in the F branch); pts1, pts2 [P,N,2] (calibrated coordinates, or image-size
        normalised ones + K1, K2, im sizes in the F branch); gt_R [P,3,3]; gt_t [P,3]; keep [P,M] bool (models to average
        over, e.g. the solver's validity flags; None = all) -> scalar loss."""
        # svd=True: decompose_E (cv_utils.py:83-116) instead of Horn's closed form; forward only (ops.pose_error)
        if self.fmat:
            estimated_models, pts1, pts2 = calibrate(estimated_models, pts1, pts2, K1, K2, im_size1, im_size2)
        matches = torch.cat((pts1, pts2), dim=-1).to(estimated_models.dtype).contiguous()
        err_R, err_t, _, _ = ops.pose_error(matches, estimated_models, gt_R, gt_t, svd=bool(svd))
        per_model = (err_R + err_t) / 2
        if keep is not None:
            k = keep.to(per_model.dtype)
            per_pair = (per_model * k).sum(1) / k.sum(1).clamp(min=1.0)
        else:
            per_pair = per_model.mean(1)
        return per_pair.mean()

    __call__ = forward_average


class ClassificationLoss(object):
    """ClassificationLoss (loss.py:71-104), essential-matrix branch: binary cross-entropy between the per-correspondence
    inlier probabilities and the inlier mask of `cv2.recoverPose(gt_E, pts1, pts2)` (here `ops.recover_pose_mask`)."""

    def __init__(self, fmat=False):
        self.fmat = fmat

    def forward(self, gt_E, matches, probs, K1=None, K2=None, im_size1=None, im_size2=None):
        """gt_E [P,3,3], matches [P,N,4] (calibrated, or image-size normalised + K1, K2, im sizes in the F branch), probs
        [P,N] in (0,1) -> scalar loss."""
        if self.fmat:
            _, p1, p2 = calibrate(gt_E[:, None], matches[..., :2], matches[..., 2:], K1, K2, im_size1, im_size2)
            matches = torch.cat((p1, p2), dim=-1).contiguous()
        with torch.no_grad():
            gt_mask = ops.recover_pose_mask(matches, gt_E)[0][:, 0]
        return torch.nn.functional.binary_cross_entropy(probs, gt_mask.to(probs.dtype))

    __call__ = forward


class _PairLoss(object):
    """What RegistrationLoss, HomographyLoss and PnPLoss share: one test-mode model per pair is promoted to [P,1,.,.] (and its keep to [P,1]),
    and without gt_mask the mask comes from the ground-truth model at the loss's threshold, under no_grad.  A subclass names its two
    ops functions."""
    _gt_mask = _loss_mean = None

    def __init__(self, threshold):
        self.threshold = threshold

    def _forward(self, models, matches, gt_model, gt_mask, keep):
        if models.dim() == 3:
            models = models[:, None]
            keep = keep if keep is None or keep.dim() == 2 else keep[:, None]
        if gt_mask is None and gt_model is not None:
            with torch.no_grad():
                gt_mask = type(self)._gt_mask(matches, gt_model.to(matches.dtype), self.threshold)[0]
        return type(self)._loss_mean(matches, gt_mask, models, self.threshold, keep)


class RegistrationLoss(_PairLoss):
    """The training loss of ransac.BatchedRegistration(train=True): the truncated squared distance of every returned model on the
    ground-truth inlier points, what MatchLoss is for E and F.  Per pair, with d2 = |R p + t - q|^2: the mean over (kept models x
    masked points) of (d2 / threshold^2 if d2 < threshold^2 else 1); then the mean over the pairs.  The loss lies in [0, 1]; a hopeless
    hypothesis contributes the constant 1 and no gradient.  Not the reference's 3-D loss (model_cl.py:586-589: the mean squared residual
    over ALL points, which ops.rigid_residual_autograd reproduces).  Value and gradient come from one pass of
    `dr_registration_loss_fused`; nothing synchronises, so a whole train step can be captured by graphs.GraphedStep."""

    _gt_mask, _loss_mean = staticmethod(ops.registration_gt_mask), staticmethod(ops.registration_loss_mean)

    def __init__(self, threshold):
        super().__init__(threshold)         # inlier DISTANCE, float or [P] (BatchedRegistration's convention)

    def forward(self, models, matches, gt_pose=None, gt_mask=None, keep=None):
        """models [P,M,4,4] (or [P,4,4]: a test-mode result), matches [P,N,6], gt_mask [P,N] bool or gt_pose [P,4,4] (the mask is then
        the points within the threshold of that pose: ops.registration_gt_mask; neither = all points), keep [P,M] bool (models to
        average over, e.g. the fit's validity; None = all) -> scalar loss, differentiable w.r.t. the models ONLY: `matches` that
        require grad are refused (pass matches.detach(); the driver's own gradient to `matches` is unaffected)."""
        return self._forward(models, matches, gt_pose, gt_mask, keep)

    __call__ = forward


def registration_errors(model, gt_pose):
    """model [...,4,4], gt_pose broadcastable to it -> (rre_deg, rte): the rotation error acos(clamp((tr(R_gt^T R) - 1) / 2, -1, 1))
    in degrees and the translation error |t - t_gt|.  Plain torch under no_grad, for evaluation (the acos is singular at the optimum:
    the training signal is RegistrationLoss)."""
    with torch.no_grad():
        R, Rg = model[..., :3, :3], gt_pose[..., :3, :3]
        c = ((Rg * R).sum((-1, -2)) - 1.0) / 2.0          # tr(Rg^T R) = sum of the entrywise products
        rre = torch.rad2deg(torch.acos(c.clamp(-1.0, 1.0)))
        rte = (model[..., :3, 3] - gt_pose[..., :3, 3]).norm(dim=-1)
        return rre, rte


class HomographyLoss(_PairLoss):
    """The training loss of ransac.BatchedHomography(train=True): the truncated symmetric transfer error of every returned model on
    the ground-truth inlier points, what RegistrationLoss is for rigid poses.  With y = H (x1, 1), z = adj(H) (x2, 1) under the
    det > 0 sign and d2 = |x2 - y_xy / y_w|^2 + |x1 - z_xy / z_w|^2 (the residual the score kernels use): per pair the mean over
    (kept models x masked points) of (d2 / threshold^2 if the point lies in front of both cameras and d2 < threshold^2, else 1); then
    the mean over the pairs.  The loss lies in [0, 1] and does not depend on the scale or the sign of a model; a hopeless hypothesis
    contributes the constant 1 and no gradient.  Value and gradient come from one pass of `dr_homography_loss_fused`; nothing
    synchronises, so a whole train step can be captured by graphs.GraphedStep."""

    _gt_mask, _loss_mean = staticmethod(ops.homography_gt_mask), staticmethod(ops.homography_loss_mean)

    def __init__(self, threshold):
        super().__init__(threshold)         # inlier DISTANCE in pixels, float or [P] (BatchedHomography's convention)

    def forward(self, models, matches, gt_H=None, gt_mask=None, keep=None):
        """models [P,M,3,3] (or [P,3,3]: a test-mode result), matches [P,N,4], gt_mask [P,N] bool or gt_H [P,3,3] (the mask is then
        the inliers of that homography at the threshold: ops.homography_gt_mask; neither = all points), keep [P,M] bool (models to
        average over, e.g. the solver's validity; None = all) -> scalar loss, differentiable w.r.t. the models ONLY: `matches` that
        require grad are refused (pass matches.detach(); the driver's own gradient to `matches` is unaffected)."""
        return self._forward(models, matches, gt_H, gt_mask, keep)

    __call__ = forward


def homography_errors(model, gt_H, size):
    """model [...,3,3], gt_H broadcastable to it, size = (h, w) of the first image -> the mean corner error in pixels: the mean over the
    corners (0, 0), (w, 0), (w, h), (0, h) of the distance between their images under the two homographies (the scale and the sign
    of either matrix do not matter).  Plain torch under no_grad, for evaluation; the training signal is HomographyLoss."""
    with torch.no_grad():
        h, w = float(size[0]), float(size[1])
        corners = torch.tensor([[0.0, 0.0, 1.0], [w, 0.0, 1.0], [w, h, 1.0], [0.0, h, 1.0]], dtype=model.dtype, device=model.device)

        def images(H):
            y = corners @ H.transpose(-1, -2)              # [...,4,3]
            return y[..., :2] / y[..., 2:]
        return (images(model) - images(gt_H.to(model.dtype))).norm(dim=-1).mean(-1)


class PnPLoss(_PairLoss):
    """The training loss of ransac.BatchedPnP.hypotheses: the truncated squared reprojection error of every returned pose on the
    ground-truth inlier points, what RegistrationLoss is for rigid registration.  With x_c = R X + t and
    d2 = (x_c / z_c - u)^2 + (y_c / z_c - v)^2 (the residual the score kernels use): per pair the mean over (kept models x masked
    points) of (d2 / threshold^2 if the point lies in front of the camera and d2 < threshold^2, else 1); then the mean over the pairs.
    The loss lies in [0, 1]; a hopeless hypothesis contributes the constant 1 and no gradient.  Value and gradient come from one pass
    of `dr_pnp_loss_fused`; nothing synchronises.  The evaluation metric on a pose is registration_errors (the model layout is the
    registration family's)."""

    _gt_mask, _loss_mean = staticmethod(ops.pnp_gt_mask), staticmethod(ops.pnp_loss_mean)

    def __init__(self, threshold):
        super().__init__(threshold)         # inlier DISTANCE in normalised units, float or [P] (BatchedPnP's convention)

    def forward(self, models, matches, gt_pose=None, gt_mask=None, keep=None):
        """models [P,M,4,4] (or [P,4,4]: a test-mode result), matches [P,N,5], gt_mask [P,N] bool or gt_pose [P,4,4] (the mask is then
        the inliers of that pose at the threshold: ops.pnp_gt_mask; neither = all points), keep [P,M] bool (models to average over,
        e.g. the solver's validity; None = all) -> scalar loss, differentiable w.r.t. the models ONLY: `matches` that require grad are
        refused (pass matches.detach(); the driver's own gradient to `matches` is unaffected)."""
        return self._forward(models, matches, gt_pose, gt_mask, keep)

    __call__ = forward


def pnp_pose_errors(models, gt_pose, trans_weight, max_loss):
    """models [P,M,4,4], gt_pose [P,4,4] -> l [P,M] = min(max(RRE in degrees, trans_weight RTE), max_loss), differentiable w.r.t. the
    models: plain torch on [P,M], as homography_errors is.  RRE = acos(c), c = (tr(Rg^T R) - 1) / 2 clamped to [-_ACOS_MAX, _ACOS_MAX],
    so a pose equal to the ground truth (derivative of acos at 1: infinite) has a rotation term of 0.081 degrees with a zero gradient.
    It is evaluated as 2 asin(sqrt(q / 2)) with q = 1 - c = |R - Rg|_F^2 / 4 (for two rotations: tr(Rg^T R) = 3 - |R - Rg|_F^2 / 2) and
    the clamp carried over to q: the same function, but c itself holds an angle of 0.2 degrees in the last two of f32's seven digits
    (1 - c = 6e-6 against an eps of 6e-8: one per cent of the angle), while q holds it in all of them."""
    D = models[..., :3, :3] - gt_pose[:, None, :3, :3]
    q = ((D * D).sum((-1, -2)) / 4.0).clamp(1.0 - _ACOS_MAX, 1.0 + _ACOS_MAX)
    rre = torch.rad2deg(2.0 * torch.asin(torch.sqrt(q / 2.0)))
    d = models[..., :3, 3] - gt_pose[:, None, :3, 3]
    rte = torch.sqrt((d * d).sum(-1) + _RTE_EPS2)         # (smooth at a zero difference)
    return torch.maximum(rre, trans_weight * rte).clamp(max=max_loss)


_ACOS_MAX = 1.0 - 1e-6
_RTE_EPS2 = 1e-24


class _ExpectedLoss(object):
    """What PnPExpectedLoss, RegistrationExpectedLoss and HomographyExpectedLoss share: the expected error of the hypotheses under a
    soft-max of their soft inlier scores.  A subclass names its score op and its defaults, and says which models are usable
    (`_usable`) and what their errors against the ground truth are (`_errors`).

        score[p,m] = the family's soft score: sum over the scored points of sigmoid(beta (1 - d2 / threshold^2))
        probs[p,:] = softmax(alpha score[p,:] / N_p) over the usable slots, N_p = the number of scored points; 0 elsewhere
        l[p,m]     = the family's error of model m against the pair's ground truth, at most max_loss
        loss       = mean over the pairs of sum_m probs l

    A slot is usable if keep holds it and the family calls its model usable.  A pair without a usable slot contributes 0 and passes
    no gradient."""
    _score_op = None                                          # the name of the family's score in ops (looked up at the call)
    _tail_f64 = False                                         # everything behind the scores in f64 whatever their type (below)

    def __init__(self, threshold, beta, alpha, max_loss):
        self.threshold, self.beta, self.alpha, self.max_loss = threshold, float(beta), float(alpha), float(max_loss)
        self.per_pair = self.probs = self.scores = None       # of the last call (detached)

    def _usable(self, models):
        """models [P,M,r,c] -> [P,M] bool: the slots whose model the family's score kernel evaluates"""
        raise NotImplementedError

    def _errors(self, models, gt):
        """models [P,M,r,c] (every slot usable), gt [P,r,c], both in the tail's type -> l [P,M], differentiable w.r.t. the models"""
        raise NotImplementedError

    def _forward(self, models, matches, gt_model, keep, mask):
        scores = getattr(ops, self._score_op)(matches, models, self.threshold, self.beta, mask, keep)
        P, M = scores.shape
        usable = self._usable(models)
        if keep is not None:
            usable = usable & keep
        # f32 logits of alpha score / N ~ 60 carry 2e-6 each, and a slot's probability and its whole gradient row carry that RELATIVE
        # error, as much again as the f32 score tensor itself brings; l - sum probs l cancels likewise.  A family that sets _tail_f64 runs
        # everything behind the scores -- [P,M]-sized torch ops -- and its backward in f64; the results and the two gradients are
        # rounded to the inputs' type once.  PnPExpectedLoss keeps the type's own arithmetic, bit for bit.
        dt = scores.dtype
        wide = torch.float64 if self._tail_f64 else dt
        n_p = matches.shape[1] if mask is None else mask.sum(1, keepdim=True).clamp(min=1).to(wide)
        # the soft-max over the usable slots, written out (exp of the logits less their largest, 0 at an unusable slot, over the sum): a
        # pair without a usable slot gets zeros, and nothing depends on how a library soft-max treats -inf or a long row
        logits = self.alpha * scores.to(wide) / n_p
        top = logits.detach().masked_fill(~usable, float("-inf")).max(1, keepdim=True).values
        top = torch.where(usable.any(1, keepdim=True), top, torch.zeros_like(top))
        e = torch.where(usable, torch.exp(logits - top), torch.zeros_like(logits))
        probs = e / e.sum(1, keepdim=True).clamp(min=torch.finfo(e.dtype).tiny)
        # an unusable slot's model (possibly NaN) is replaced BEFORE the errors: a NaN behind a where() would still poison its gradient
        eye = torch.eye(models.shape[-1], device=models.device, dtype=models.dtype)
        errors = self._errors(torch.where(usable[:, :, None, None], models, eye).to(wide), gt_model.to(wide))
        per_pair = (probs * errors).sum(1).to(dt)
        probs = probs.to(dt)
        self.per_pair, self.probs, self.scores = per_pair.detach(), probs.detach(), scores.detach()
        return per_pair.mean()


class _PoseExpectedLoss(_ExpectedLoss):
    """The two families on the [P,M,4,4] pose layout: a model is usable if its twelve entries are finite, and its error is
    l = min(max(RRE in degrees, trans_weight RTE), max_loss) against gt_pose (pnp_pose_errors)."""

    def __init__(self, threshold, beta, alpha, trans_weight, max_loss):
        super().__init__(threshold, beta, alpha, max_loss)
        self.trans_weight = float(trans_weight)

    def _usable(self, models):
        return torch.isfinite(models[:, :, :3]).all(-1).all(-1)

    def _errors(self, models, gt):
        return pnp_pose_errors(models, gt, self.trans_weight, self.max_loss)


class PnPExpectedLoss(_PoseExpectedLoss):
    """The DSAC / DSAC* training loss on ransac.BatchedPnP.hypotheses: the expected pose error of the hypotheses under a soft-max of
    their soft inlier scores.  It needs no ground-truth inlier mask, weights a hypothesis by how many points agree with it, and gives
    a gradient to `matches` -- whose 3-D column is a network output in scene-coordinate regression -- through the minimal solver (the
    models) and through the scores.

        score[p,m] = ops.pnp_soft_score: sum over the scored points of sigmoid(beta (1 - d2 / threshold^2))
        probs[p,:] = softmax(alpha score[p,:] / N_p) over the usable slots, N_p = the number of scored points; 0 elsewhere
        l[p,m]     = min(max(RRE in degrees, trans_weight RTE), max_loss) against gt_pose            (pnp_pose_errors)
        loss       = mean over the pairs of sum_m probs l

    A slot is usable if keep holds it and its model is finite.  A pair without a usable slot contributes 0 and passes no gradient.
    Defaults: DSAC*'s published hyper-parameters (Brachmann and Rother, TPAMI 2021) restated for this package's units.  DSAC* scores
    with sigmoid(beta_px (tau - r)) on the reprojection error r in pixels, tau = 10 px and beta_px = 0.5 / px, so beta_px tau = 5
    = `beta` here, the weight's slope in units of the threshold, whatever the threshold's unit; the threshold itself is the driver's,
    in normalised units (10 px / f), and the error enters SQUARED (the package's convention).  alpha = 100 is DSAC*'s
    inlier alpha on the score divided by the number of points.  DSAC* compares degrees with centimetres: trans_weight = 100 for a
    scene in metres, and clamps the pose loss at 100; both are kept.  They are hyper-parameters, not tuned here."""

    _score_op = "pnp_soft_score"

    def __init__(self, threshold, beta=5.0, alpha=100.0, trans_weight=100.0, max_loss=100.0):
        super().__init__(threshold, beta, alpha, trans_weight, max_loss)

    def forward(self, models, matches, gt_pose, keep=None, mask=None):
        """models [P,M,4,4], matches [P,N,5] (they MAY require grad), gt_pose [P,4,4], keep [P,M] bool (e.g. hypotheses' keep; None =
        all), mask [P,N] bool (the points that are scored; None = all) -> scalar loss.  The per-pair values, the probabilities and the
        scores of the call stay on the object as .per_pair [P], .probs [P,M], .scores [P,M], detached."""
        return self._forward(models, matches, gt_pose, keep, mask)

    __call__ = forward


class RegistrationExpectedLoss(_PoseExpectedLoss):
    """The DSAC training loss on ransac.BatchedRegistration(train=True): PnPExpectedLoss's definition on the registration family's
    soft score (ops.registration_soft_score, d2 = |R p + t - q|^2).  Unlike RegistrationLoss it needs no ground-truth inlier mask,
    weights a hypothesis by how many correspondences agree with it instead of averaging the kept ones equally, and gives a gradient
    to `matches` through the minimal solver (the models) and through the scores.

        score[p,m] = ops.registration_soft_score: sum over the scored points of sigmoid(beta (1 - d2 / threshold^2))
        probs[p,:] = softmax(alpha score[p,:] / N_p) over the usable slots, N_p = the number of scored points; 0 elsewhere
        l[p,m]     = min(max(RRE in degrees, trans_weight RTE), max_loss) against gt_pose            (pnp_pose_errors)
        loss       = mean over the pairs of sum_m probs l

    A slot is usable if keep holds it and its model is finite.  A pair without a usable slot contributes 0 and passes no gradient.
    Defaults: beta = 5, alpha = 100 and max_loss = 100 are PnPExpectedLoss's (DSAC*'s, restated in units of the threshold); the
    threshold is the driver's inlier distance.  trans_weight = 50 sets one degree against 2 cm, the ratio of the usual 3DMatch recall
    criterion (15 degrees and 0.3 m).  All of them are hyper-parameters, not tuned here.  What follows the scores (the soft-max, the
    pose errors, the sums: [P,M]-sized) and its backward run in f64 whatever the type of the inputs (_ExpectedLoss._forward says why);
    the results and the gradients are rounded to that type once."""

    _score_op = "registration_soft_score"
    _tail_f64 = True

    def __init__(self, threshold, beta=5.0, alpha=100.0, trans_weight=50.0, max_loss=100.0):
        super().__init__(threshold, beta, alpha, trans_weight, max_loss)

    def forward(self, models, matches, gt_pose, keep=None, mask=None):
        """models [P,M,4,4], matches [P,N,6] (they MAY require grad), gt_pose [P,4,4], keep [P,M] bool (e.g. the driver's keep; None =
        all), mask [P,N] bool (the points that are scored; None = all) -> scalar loss.  The per-pair values, the probabilities and the
        scores of the call stay on the object as .per_pair [P], .probs [P,M], .scores [P,M], detached."""
        return self._forward(models, matches, gt_pose, keep, mask)

    __call__ = forward


_CORNER_EPS2 = 1e-12


def _det3(m):
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1])
            - m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0])
            + m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """a b = p + e exactly (Dekker's product on Veltkamp's split: torch has no fused multiply-add to ask the remainder of)"""
    def split(x):
        c = 134217729.0 * x
        hi = c - (c - x)
        return hi, x - hi
    p = a * b
    (ah, al), (bh, bl) = split(a), split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _corner_images(H, corners):
    """H [...,3,3], corners [4,3] = (x, y, 1), f64 -> (t, t_lo, w): the images H (x, y, 1)_xy / w of the corners as hi + lo
    [...,4,2] and w [...,4] (replaced by 1 where it is not positive, BEFORE the division).  Every linear form is summed error-free
    and the quotient is corrected by its remainder: an image of hundreds of pixels is good to an eps of an eps of itself."""
    def form(r):                                           # H[r,0] x + H[r,1] y + H[r,2]
        p0, e0 = _two_prod(H[..., None, r, 0], corners[:, 0])
        p1, e1 = _two_prod(H[..., None, r, 1], corners[:, 1])
        s, es0 = _two_sum(p0, p1)
        hi, es1 = _two_sum(s, H[..., None, r, 2].expand_as(s))
        return hi, (e0 + e1) + (es0 + es1)
    (x, xl), (y, yl), (w, wl) = form(0), form(1), form(2)
    back = ~(w > 0)
    w, wl = torch.where(back, torch.ones_like(w), w), torch.where(back, torch.zeros_like(wl), wl)

    def quotient(n, nl):
        q = n / w
        p, e = _two_prod(q, w)
        return q, (((n - p) - e) + (nl - q * wl)) / w
    (tx, txl), (ty, tyl) = quotient(x, xl), quotient(y, yl)
    return torch.stack((tx, ty), -1), torch.stack((txl, tyl), -1), torch.where(back, torch.zeros_like(w), w)


def homography_corner_errors(models, gt_H, size, max_loss):
    """models [P,M,3,3] (finite, det != 0), gt_H [P,3,3], size = (h, w) of the first image (homography_errors' convention) -> l [P,M] =
    min(mean corner error in pixels, max_loss), differentiable w.r.t. the models: plain torch on [P,M], what pnp_pose_errors is for
    poses.  The corner error is homography_errors' -- the mean over the corners (0, 0), (w, 0), (w, h), (0, h) of the distance between
    their images under the two homographies -- with each distance as sqrt(|d|^2 + 1e-12) (smooth at a zero difference: within a
    millionth of a pixel of it the direction d / |d| of the plain norm's gradient is made of roundings).  A model that sends any of
    the four corners to w <= 0 under the det > 0 sign (the sign the score kernels evaluate it under) maps the image through infinity:
    it takes l = max_loss and no gradient; the division is guarded by a where() BEFORE it, so no NaN reaches a gradient.
    d is the difference of two images of hundreds of pixels and, for a good hypothesis, a fraction of a pixel itself; its direction
    d / |d| is the whole gradient, and in plain f64 it would carry 1e-13 / |d|, more than an ulp of the inputs moves it.  So the VALUE of d
    is formed in f64 beyond its precision whatever the type of the models (_corner_images: hi + lo images, differenced exactly),
    while its derivative, which cancels nothing, is autograd's of the plain expression."""
    h, w = float(size[0]), float(size[1])
    corners = torch.tensor([[0.0, 0.0, 1.0], [w, 0.0, 1.0], [w, h, 1.0], [0.0, h, 1.0]], dtype=models.dtype, device=models.device)
    det = _det3(models.detach())
    sign = torch.where(det < 0, -torch.ones_like(det), torch.ones_like(det))
    y = torch.einsum("pmij,cj->pmci", models * sign[..., None, None], corners)         # [P,M,4,3]
    front = y[..., 2] > 0
    yw = torch.where(front, y[..., 2], torch.ones_like(y[..., 2]))
    g = torch.einsum("pij,cj->pci", gt_H.to(models.dtype), corners)                    # [P,4,3]
    d = y[..., :2] / yw[..., None] - (g[..., :2] / g[..., 2:])[:, None]
    with torch.no_grad():
        c64 = corners.double()
        t, tl, tw = _corner_images((models * sign[..., None, None]).double(), c64)
        u, ul, _ = _corner_images(gt_H.double()[:, None], c64)
        s, e = _two_sum(t, -u.expand_as(t))
        exact = (s + (e + (tl - ul))).to(models.dtype)
        front = front & (tw > 0)
    d = d + (torch.where(front[..., None], exact, d) - d).detach()
    err = torch.sqrt((d * d).sum(-1) + _CORNER_EPS2).mean(-1).clamp(max=max_loss)
    return torch.where(front.all(-1), err, torch.full_like(err, max_loss))


class HomographyExpectedLoss(_ExpectedLoss):
    """The DSAC training loss on ransac.BatchedHomography(train=True): the expected corner error of the hypotheses under a soft-max of
    their soft inlier scores (ops.homography_soft_score, d2 = the squared symmetric transfer error).  Unlike HomographyLoss it needs
    no ground-truth inlier mask, weights a hypothesis by how many matches agree with it instead of averaging the kept ones equally,
    and gives a gradient to `matches` through the minimal solver (the models) and through the scores.

        score[p,m] = ops.homography_soft_score: sum over the scored points of sigmoid(beta (1 - d2 / threshold^2))
        probs[p,:] = softmax(alpha score[p,:] / N_p) over the usable slots, N_p = the number of scored points; 0 elsewhere
        l[p,m]     = min(mean corner error in pixels of H_m against gt_H, max_loss)                  (homography_corner_errors)
        loss       = mean over the pairs of sum_m probs l

    A slot is usable if keep holds it, its model is finite and det != 0 (the score kernel's usable set).  A usable model that sends a
    corner of the image to w <= 0 takes l = max_loss and no gradient through l.  A pair without a usable slot contributes 0 and passes
    no gradient.  `size` = (h, w) of the first image, homography_errors' convention; the threshold is the driver's inlier distance in
    pixels.  Defaults: beta = 5 and alpha = 100 are PnPExpectedLoss's (DSAC*'s, restated in units of the threshold), max_loss = 100
    pixels is DSAC*'s clamp of 100 carried to this family's unit; they are stated, not tuned here.  What follows the scores (the
    soft-max, the corner errors, the sums: [P,M]-sized) and its backward run in f64 whatever the type of the inputs
    (_ExpectedLoss._forward says why); the results and the gradients are rounded to that type once."""

    _score_op = "homography_soft_score"
    _tail_f64 = True

    def __init__(self, threshold, size, beta=5.0, alpha=100.0, max_loss=100.0):
        super().__init__(threshold, beta, alpha, max_loss)
        self.size = (float(size[0]), float(size[1]))

    def _usable(self, models):
        det = _det3(models)
        return torch.isfinite(models).all(-1).all(-1) & torch.isfinite(det) & (det != 0)

    def _errors(self, models, gt):
        return homography_corner_errors(models, gt, self.size, self.max_loss)

    def forward(self, models, matches, gt_H, keep=None, mask=None):
        """models [P,M,3,3], matches [P,N,4] (they MAY require grad), gt_H [P,3,3], keep [P,M] bool (e.g. the driver's keep; None =
        all), mask [P,N] bool (the points that are scored; None = all) -> scalar loss.  The per-pair values, the probabilities and the
        scores of the call stay on the object as .per_pair [P], .probs [P,M], .scores [P,M], detached."""
        return self._forward(models, matches, gt_H, keep, mask)

    __call__ = forward
