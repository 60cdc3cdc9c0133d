"""CPU oracle: restatement of the adversarial generators behind AddNoise (torch-CPU fp32).

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Paths cited are relative to
/root/reference/RobustART/noise/utils/adv/.

Every attack takes ``grad_fn(x) -> (logits, loss_indiv, grad)`` style callables built from a
torch model on CPU (autograd is plumbing here, the arithmetic under test is the
step/projection/bookkeeping), and takes its random start as an explicit tensor so the HIP
path can be driven with the same draws.

Pinned against unmodified reference code (tests/golden/make_golden.py): apgd (Linf, L2, ce and
dlr), apgd_targeted, mim_linf.  UNPINNED (foolbox 3.3.1 is not installed, the reference has no
tests): pgd_linf, pgd_l2, fgsm -- these follow foolbox's BaseGradientDescent.run as recalled in
SURVEY.md Appendix B, and are cross-checked only through identities (||delta|| <= eps, range).
"""
import math

import torch
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def normalize(x):
    """Attacks/imfgsm_attack.py:14-23 / Attacks/autoattack/autoattack.py:17-20."""
    mean = torch.tensor(IMAGENET_MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std


def _grad_of_sum(loss_fn, model_fn, x, y, eot_iter=1):
    """autopgd_base.py:271-289 / :367-384: the gradient averaged over eot_iter passes (logits / losses of the last one)."""
    x = x.detach().clone().requires_grad_(True)
    g = torch.zeros_like(x)
    for _ in range(eot_iter):
        with torch.enable_grad():
            logits = model_fn(x)
            loss_indiv = loss_fn(logits, y)
            loss = loss_indiv.sum()
        g += torch.autograd.grad(loss, [x])[0].detach()
    g /= float(eot_iter)
    return logits.detach(), loss_indiv.detach(), g


def ce_indiv(logits, y):
    return F.cross_entropy(logits, y, reduction='none')


# ---------------------------------------------------------------------------------------
# foolbox 3.3.1 BaseGradientDescent (attack.py:20-33) -- UNPINNED
# ---------------------------------------------------------------------------------------

def pgd_linf_step(x, g, x0, eps, stepsize):
    x = x + stepsize * torch.sign(g)
    x = x0 + torch.clamp(x - x0, -eps, eps)
    return torch.clamp(x, 0.0, 1.0)


def pgd_linf(model_fn, x0, y, eps, rel_stepsize, steps, init_u=None, random_start=True):
    """attack.py:20-23.  init_u: the U(-eps, eps) start perturbation (same shape as x0)."""
    stepsize = rel_stepsize * eps
    x = x0.clone()
    if random_start:
        x = torch.clamp(x0 + init_u, 0.0, 1.0)
    for _ in range(steps):
        _, _, g = _grad_of_sum(ce_indiv, model_fn, x, y)
        x = pgd_linf_step(x, g, x0, eps, stepsize)
    return x


def fgsm(model_fn, x0, y, eps):
    """attack.py:30-33: LinfFastGradientAttack = 1 step of size eps, no random start."""
    return pgd_linf(model_fn, x0, y, eps, 1.0, 1, random_start=False)


def _l2norms(v):
    return v.flatten(1).norm(dim=1).view(-1, 1, 1, 1)


def pgd_l2_step(x, g, x0, eps, stepsize):
    g = g / torch.clamp(_l2norms(g), min=1e-12)
    x = x + stepsize * g
    d = x - x0
    factor = torch.clamp(eps / torch.clamp(_l2norms(d), min=1e-12), max=1.0)
    x = x0 + d * factor
    return torch.clamp(x, 0.0, 1.0)


def l2_ball_start(gauss_np2, eps):
    """foolbox L2 random start: uniform point in the eps-ball from an (n+2)-dim gaussian
    (B, n+2) -> normalise -> keep first n coordinates."""
    s = gauss_np2 / gauss_np2.norm(dim=1, keepdim=True)
    return eps * s[:, :-2]


def pgd_l2(model_fn, x0, y, eps, rel_stepsize, steps, init_delta=None, random_start=True):
    """attack.py:25-28.  init_delta: start perturbation inside the eps-ball, shaped like x0."""
    stepsize = rel_stepsize * eps
    x = x0.clone()
    if random_start:
        x = torch.clamp(x0 + init_delta, 0.0, 1.0)
    for _ in range(steps):
        _, _, g = _grad_of_sum(ce_indiv, model_fn, x, y)
        x = pgd_l2_step(x, g, x0, eps, stepsize)
    return x


# ---------------------------------------------------------------------------------------
# MIM (Attacks/imfgsm_attack.py:62-93) -- pinned
# ---------------------------------------------------------------------------------------

def mim_step(x, g, m, x0, eps, step_size, decay):
    """imfgsm_attack.py:85-90."""
    g = g / torch.mean(torch.abs(g), [1, 2, 3], keepdim=True)
    m = decay * m + g
    x = x + step_size * m.sign()
    x = x0 + torch.clamp(x - x0, -eps, eps)
    return torch.clamp(x, 0.0, 1.0), m


def mim_linf(model, X, y, epsilon, num_steps, step_size, decay_factor, init_noise):
    """`model` takes NORMALISED input (imfgsm_attack.py:69,83); CE mean loss (:83);
    the start X + U(-eps,eps) is not clipped before the first forward (:73-74)."""
    x = X + init_noise
    m = torch.zeros_like(X)
    for _ in range(num_steps):
        xr = x.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            loss = F.cross_entropy(model(normalize(xr)), y)
        g = torch.autograd.grad(loss, [xr])[0].detach()
        x, m = mim_step(x, g, m, X, epsilon, step_size, decay_factor)
    return x


# ---------------------------------------------------------------------------------------
# AutoPGD (Attacks/autoattack/autopgd_base.py) -- pinned
# ---------------------------------------------------------------------------------------

def dlr_loss(x, y):
    """autopgd_base.py:198-204."""
    x_sorted, ind_sorted = x.sort(dim=1)
    ind = (ind_sorted[:, -1] == y).float()
    u = torch.arange(x.shape[0])
    return -(x[u, y] - x_sorted[:, -2] * ind - x_sorted[:, -1] * (1. - ind)) / (
        x_sorted[:, -1] - x_sorted[:, -3] + 1e-12)


def dlr_loss_targeted(x, y, y_target):
    """autopgd_base.py:599-604."""
    x_sorted, _ = x.sort(dim=1)
    u = torch.arange(x.shape[0])
    return -(x[u, y] - x[u, y_target]) / (x_sorted[:, -1] - .5 * (x_sorted[:, -3] + x_sorted[:, -4]) + 1e-12)


def _apgd_normalize(x, norm):
    """autopgd_base.py:177-184."""
    nd = x.dim() - 1
    if norm == 'Linf':
        t = x.abs().reshape(x.shape[0], -1).max(1)[0]
    else:
        t = (x ** 2).reshape(x.shape[0], -1).sum(-1).sqrt()
    return x / (t.view(-1, *([1] * nd)) + 1e-12)


def _apgd_lp_norm(x):
    """autopgd_base.py:193-196 (L2)."""
    nd = x.dim() - 1
    return (x ** 2).reshape(x.shape[0], -1).sum(-1).sqrt().view(-1, *([1] * nd))


def apgd_checkpoints(n_iter):
    """autopgd_base.py:163-165."""
    return max(int(0.22 * n_iter), 1), max(int(0.06 * n_iter), 1), max(int(0.03 * n_iter), 1)


def apgd_step_linf(x_adv, x_adv_old, grad, x, eps, step_size, a):
    """autopgd_base.py:327-338; returns (x_new, x_adv_old_new)."""
    grad2 = x_adv - x_adv_old
    x_adv_1 = x_adv + step_size * torch.sign(grad)
    x_adv_1 = torch.clamp(torch.min(torch.max(x_adv_1, x - eps), x + eps), 0.0, 1.0)
    x_adv_1 = torch.clamp(torch.min(torch.max(x_adv + (x_adv_1 - x_adv) * a + grad2 * (1 - a),
                                              x - eps), x + eps), 0.0, 1.0)
    return x_adv_1


def apgd_step_l2(x_adv, x_adv_old, grad, x, eps, step_size, a):
    """autopgd_base.py:340-348."""
    grad2 = x_adv - x_adv_old
    x_adv_1 = x_adv + step_size * _apgd_normalize(grad, 'L2')
    x_adv_1 = torch.clamp(x + _apgd_normalize(x_adv_1 - x, 'L2') * torch.min(
        eps * torch.ones_like(x), _apgd_lp_norm(x_adv_1 - x)), 0.0, 1.0)
    x_adv_1 = x_adv + (x_adv_1 - x_adv) * a + grad2 * (1 - a)
    x_adv_1 = torch.clamp(x + _apgd_normalize(x_adv_1 - x, 'L2') * torch.min(
        eps * torch.ones_like(x), _apgd_lp_norm(x_adv_1 - x)), 0.0, 1.0)
    return x_adv_1


def apgd_single_run(model_fn, x, y, norm, eps, n_iter, loss, init_t, y_target=None, rho=0.75, trace=None, eot_iter=1):
    """autopgd_base.py:208-448 (eot_iter = 1, Linf / L2).  init_t = the torch.rand*2-1 (Linf)
    or torch.randn (L2) start direction.  Returns (x_best, acc, loss_best, x_best_adv)."""
    if loss == 'ce':
        crit = ce_indiv
    elif loss == 'dlr':
        crit = dlr_loss
    elif loss == 'dlr-targeted':
        crit = lambda lg, yy: dlr_loss_targeted(lg, yy, y_target)
    else:
        raise ValueError(loss)
    nd = x.dim() - 1
    n_iter_2, n_iter_min, size_decr = apgd_checkpoints(n_iter)

    x_adv = x + eps * torch.ones_like(x) * _apgd_normalize(init_t, norm)       # :213-220
    x_adv = x_adv.clamp(0., 1.)                                                # :237
    x_best = x_adv.clone()
    x_best_adv = x_adv.clone()
    B = x.shape[0]
    loss_steps = torch.zeros([n_iter, B])

    logits, loss_indiv, grad = _grad_of_sum(crit, model_fn, x_adv, y, eot_iter)          # :271-289
    grad_best = grad.clone()
    acc = logits.max(1)[1] == y
    loss_best = loss_indiv.clone()
    step_size = 2. * eps * torch.ones([B, *([1] * nd)])                        # :296-298
    x_adv_old = x_adv.clone()
    k = n_iter_2 + 0
    counter3 = 0
    loss_best_last_check = loss_best.clone()
    reduced_last_check = torch.ones_like(loss_best)

    for i in range(n_iter):
        x_adv = x_adv.detach()
        a = 0.75 if i > 0 else 1.0
        step = apgd_step_linf if norm == 'Linf' else apgd_step_l2
        x_new = step(x_adv, x_adv_old, grad, x, eps, step_size, a)
        x_adv_old = x_adv.clone()
        x_adv = x_new + 0.

        logits, loss_indiv, grad = _grad_of_sum(crit, model_fn, x_adv, y, eot_iter)      # :367-384
        pred = logits.max(1)[1] == y
        acc = torch.min(acc, pred)
        ind_pred = ~pred
        x_best_adv[ind_pred] = x_adv[ind_pred] + 0.                            # :389-390

        y1 = loss_indiv.clone()                                                # :399-406
        loss_steps[i] = y1 + 0
        ind = y1 > loss_best
        x_best[ind] = x_adv[ind].clone()
        grad_best[ind] = grad[ind].clone()
        loss_best[ind] = y1[ind] + 0
        if trace is not None:
            trace.append(dict(x_adv=x_adv.clone(), grad=grad.clone(), loss=y1.clone(),
                              step_size=step_size.flatten().clone()))
        counter3 += 1
        if counter3 == k:                                                      # :410-429
            t = torch.zeros(B)
            for c5 in range(k):                                                # check_oscillation :167-172
                t += (loss_steps[i - c5] > loss_steps[i - c5 - 1]).float()
            fl_osc = (t <= k * rho * torch.ones_like(t)).float()
            fl_no_impr = (1. - reduced_last_check) * (loss_best_last_check >= loss_best).float()
            fl_osc = torch.max(fl_osc, fl_no_impr)
            reduced_last_check = fl_osc.clone()
            loss_best_last_check = loss_best.clone()
            if fl_osc.sum() > 0:
                sel = fl_osc > 0
                step_size[sel] /= 2.0
                x_adv[sel] = x_best[sel].clone()
                grad[sel] = grad_best[sel].clone()
            k = max(k - size_decr, n_iter_min)
            counter3 = 0
    return x_best, acc, loss_best, x_best_adv


# ---------------------------------------------------------------------------------------
# APGD, L1 threat model (autopgd_base.py:19-83 L1_projection; :222-226, :300-313, :351-364, :431-441, :531-555) -- pinned
# ---------------------------------------------------------------------------------------

def l1_projection(x2, y2, eps1):
    """autopgd_base.py:19-83: delta such that ||y2 + delta||_1 <= eps1 and 0 <= x2 + y2 + delta <= 1 (the exact projection
    onto the intersection of the L1 ball around x2 and the box).  Per coordinate the perturbation magnitude |y| shrinks by
    clip(alpha, -u, |y|), u = min(min(1 - x - y, x + y), 0) being what the box alone demands; alpha is the root of the
    piecewise-linear budget equation, found on the sorted breakpoints."""
    dt = torch.float64 if x2.dtype == torch.float64 and y2.dtype == torch.float64 else torch.float32      # fp64 in, fp64 throughout
    x = x2.clone().to(dt).reshape(x2.shape[0], -1)
    y = y2.clone().to(dt).reshape(y2.shape[0], -1)
    sigma = y.clone().sign()
    u = torch.min(1 - x - y, x + y)
    u = torch.min(torch.zeros_like(y), u)
    l = -torch.clone(y).abs()
    d = u.clone()
    bs, indbs = torch.sort(-torch.cat((u, l), 1), dim=1)
    bs2 = torch.cat((bs[:, 1:], torch.zeros(bs.shape[0], 1)), 1)
    inu = 2 * (indbs < u.shape[1]).float() - 1
    size1 = inu.cumsum(dim=1)
    s1 = -u.sum(dim=1)
    c = eps1 - y.clone().abs().sum(dim=1)
    c5 = s1 + c < 0
    c2 = c5.nonzero().squeeze(1)
    s = s1.unsqueeze(-1) + torch.cumsum((bs2 - bs) * size1, dim=1)
    if c2.numel() != 0:
        lb = torch.zeros_like(c2).float()
        ub = torch.ones_like(lb) * (bs.shape[1] - 1)
        nitermax = torch.ceil(torch.log2(torch.tensor(bs.shape[1]).float()))
        counter = 0
        while counter < nitermax:
            counter4 = torch.floor((lb + ub) / 2.)
            counter2 = counter4.long()
            c8 = s[c2, counter2] + c[c2] < 0
            lb = torch.where(c8, counter4, lb)
            ub = torch.where(c8, ub, counter4)
            counter += 1
        lb2 = lb.long()
        alpha = (-s[c2, lb2] - c[c2]) / size1[c2, lb2 + 1] + bs2[c2, lb2]
        d[c2] = -torch.min(torch.max(-u[c2], alpha.unsqueeze(-1)), -l[c2])
    return (sigma * d).view(x2.shape)


def _l0(x):
    return (x != 0.).reshape(x.shape[0], -1).sum(-1)


def apgd_l1_single_run(model_fn, x, y, eps, n_iter, loss, init_t=None, x_init=None, y_target=None, trace=None):
    """attack_single_run with norm = 'L1' (autopgd_base.py:208-448): start x + t + L1_projection(x, t, eps) from
    t = randn (:222-226) or a given x_init (:230-234); sparse sign steps on the top-k gradient entries (:351-364); every
    k = max(int(0.04 n_iter), 1) iterations the sparsity / step size adaptation of :431-441.  Returns
    (x_best, acc, loss_best, x_best_adv)."""
    crit = {'ce': ce_indiv, 'dlr': dlr_loss}.get(loss) or (lambda lg, yy: dlr_loss_targeted(lg, yy, y_target))
    nd = x.dim() - 1
    B = x.shape[0]
    n_fts = x[0].numel()
    if x_init is None:
        x_adv = x + init_t + l1_projection(x, init_t, eps)
    else:
        x_adv = x_init.clone()
    x_adv = x_adv.clamp(0., 1.)
    x_best = x_adv.clone()
    x_best_adv = x_adv.clone()
    logits, loss_indiv, grad = _grad_of_sum(crit, model_fn, x_adv, y)
    grad_best = grad.clone()
    acc = logits.max(1)[1] == y
    loss_best = loss_indiv.clone()
    alpha = 1.
    step_size = alpha * eps * torch.ones([B, *([1] * nd)])
    k = max(int(.04 * n_iter), 1)
    if x_init is None:
        topk = .2 * torch.ones([B])
        sp_old = n_fts * torch.ones_like(topk)
    else:
        topk = _l0(x_adv - x) / n_fts / 1.5
        sp_old = _l0(x_adv - x)
    adasp_redstep, adasp_minstep = 1.5, 10.
    counter3 = 0
    u = torch.arange(B)
    for i in range(n_iter):
        x_adv = x_adv.detach()
        grad_topk = grad.abs().reshape(B, -1).sort(-1)[0]
        topk_curr = torch.clamp((1. - topk) * n_fts, min=0, max=n_fts - 1).long()
        grad_topk = grad_topk[u, topk_curr].view(-1, *[1] * nd)
        sparsegrad = grad * (grad.abs() >= grad_topk).float()
        x_adv_1 = x_adv + step_size * sparsegrad.sign() / (
            sparsegrad.sign().abs().reshape(B, -1).sum(dim=-1).view(-1, *[1] * nd) + 1e-10)
        delta_u = x_adv_1 - x
        delta_p = l1_projection(x, delta_u, eps)
        x_adv = x + delta_u + delta_p

        logits, loss_indiv, grad = _grad_of_sum(crit, model_fn, x_adv, y)
        pred = logits.max(1)[1] == y
        acc = torch.min(acc, pred)
        x_best_adv[~pred] = x_adv[~pred] + 0.
        y1 = loss_indiv.clone()
        ind = y1 > loss_best
        x_best[ind] = x_adv[ind].clone()
        grad_best[ind] = grad[ind].clone()
        loss_best[ind] = y1[ind] + 0
        if trace is not None:
            trace.append(dict(x_adv=x_adv.clone(), grad=grad.clone(), loss=y1.clone(), step_size=step_size.flatten().clone(),
                              topk=topk.clone()))
        counter3 += 1
        if counter3 == k:
            sp_curr = _l0(x_best - x)
            fl_redtopk = (sp_curr / sp_old) < .95
            topk = sp_curr / n_fts / 1.5
            step_size[fl_redtopk] = alpha * eps
            step_size[~fl_redtopk] /= adasp_redstep
            step_size.clamp_(alpha * eps / adasp_minstep, alpha * eps)
            sp_old = sp_curr.clone()
            x_adv[fl_redtopk] = x_best[fl_redtopk].clone()
            grad[fl_redtopk] = grad_best[fl_redtopk].clone()
            counter3 = 0
    return x_best, acc, loss_best, x_best_adv


def apgd_l1_largereps_schedule(eps, n_iter):
    """autopgd_base.py:490-495: (epss, iters) of the decreasing-radius schedule used when use_largereps is set."""
    epss = [3. * eps, 2. * eps, 1. * eps]
    iters = [math.ceil(.3 * n_iter), math.ceil(.3 * n_iter), math.ceil(.4 * n_iter)]
    iters[-1] = n_iter - sum(iters[:-1])
    return epss, iters


def apgd_l1_decr_eps(model_fn, x, y, eps, n_iter, loss, init_noise, y_target=None):
    """decr_eps_pgd (autopgd_base.py:531-555): x_init = x + randn, projected onto the 3 eps ball, then three runs with
    radii 3 eps, 2 eps, eps, each started from the previous best point re-projected.  init_noise = the torch.randn_like(x)."""
    epss, iters = apgd_l1_largereps_schedule(eps, n_iter)
    x_init = x + init_noise
    x_init = x_init + l1_projection(x, x_init, 1. * float(epss[0]))      # (sic: the reference passes x_init, not x_init - x)
    for e, nit in zip(epss, iters):
        x_init = x_init + l1_projection(x, x_init - x, e)
        x_init, acc, loss_b, x_adv = apgd_l1_single_run(model_fn, x, y, e, nit, loss, x_init=x_init, y_target=y_target)
    return x_init, acc, loss_b, x_adv


def apgd_l1_perturb(model_fn, x, y, eps, n_iter, loss, draws, n_restarts=1, use_largereps=False):
    """APGDAttack.perturb with norm = 'L1' (autopgd_base.py:450-529).  draws(counter, shape) supplies the torch.randn of
    restart `counter` for the still-robust subset (randn for a plain run, randn_like for the larger-eps schedule)."""
    x = x.detach().clone().float()
    y_pred = model_fn(x).max(1)[1]
    adv = x.clone()
    acc = y_pred == y
    for counter in range(n_restarts):
        ind = acc.nonzero().flatten()
        if ind.numel() != 0:
            xs, ys = x[ind].clone(), y[ind].clone()
            t = draws(counter, xs.shape)
            if use_largereps:
                _, acc_curr, _, adv_curr = apgd_l1_decr_eps(model_fn, xs, ys, eps, n_iter, loss, t)
            else:
                _, acc_curr, _, adv_curr = apgd_l1_single_run(model_fn, xs, ys, eps, n_iter, loss, init_t=t)
            ind_curr = (acc_curr == 0).nonzero().flatten()
            acc[ind[ind_curr]] = False
            adv[ind[ind_curr]] = adv_curr[ind_curr].clone()
    return adv


def apgd_perturb(model_fn, x, y, norm, eps, n_iter, loss, init_ts, n_restarts=1, eot_iter=1):
    """autopgd_base.py:450-529 (best_loss=False).  init_ts[r] = start direction for restart r,
    shaped like the still-robust subset at that restart."""
    x = x.detach().clone().float()
    y_pred = model_fn(x).max(1)[1]
    adv = x.clone()
    acc = y_pred == y
    for counter in range(n_restarts):
        ind_to_fool = acc.nonzero().flatten()
        if ind_to_fool.numel() != 0:
            t = init_ts(counter, x[ind_to_fool].shape) if callable(init_ts) else init_ts[counter]
            _, acc_curr, _, adv_curr = apgd_single_run(model_fn, x[ind_to_fool].clone(), y[ind_to_fool].clone(),
                                                       norm, eps, n_iter, loss, t, eot_iter=eot_iter)
            ind_curr = (acc_curr == 0).nonzero().flatten()
            acc[ind_to_fool[ind_curr]] = False
            adv[ind_to_fool[ind_curr]] = adv_curr[ind_curr].clone()
    return adv


def apgd_targeted_perturb(model_fn, x, y, norm, eps, n_iter, init_ts, n_target_classes=9):
    """autopgd_base.py:610-690 (n_restarts = 1).  init_ts[j] for target_class j+2."""
    x = x.detach().clone().float()
    y_pred = model_fn(x).max(1)[1]
    adv = x.clone()
    acc = y_pred == y
    for j, target_class in enumerate(range(2, n_target_classes + 2)):
        ind_to_fool = acc.nonzero().flatten()
        if ind_to_fool.numel() != 0:
            x_to_fool = x[ind_to_fool].clone()
            y_to_fool = y[ind_to_fool].clone()
            output = model_fn(x_to_fool)
            y_target = output.sort(dim=1)[1][:, -target_class]
            t = init_ts(j, x_to_fool.shape) if callable(init_ts) else init_ts[j]
            _, acc_curr, _, adv_curr = apgd_single_run(model_fn, x_to_fool, y_to_fool, norm, eps, n_iter,
                                                       'dlr-targeted', t, y_target=y_target)
            ind_curr = (acc_curr == 0).nonzero().flatten()
            acc[ind_to_fool[ind_curr]] = False
            adv[ind_to_fool[ind_curr]] = adv_curr[ind_curr].clone()
    return adv


# ---------------------------------------------------------------------------------------
# Square attack, Linf (Attacks/autoattack/square.py:68-86,192-294,532-600) -- pinned
# ---------------------------------------------------------------------------------------

def square_p_selection(it, p_init, n_queries, rescale):
    """square.py:192-219."""
    if rescale:
        it = int(it / n_queries * 10000)
    if 10 < it <= 50:
        return p_init / 2
    if 50 < it <= 200:
        return p_init / 4
    if 200 < it <= 500:
        return p_init / 8
    if 500 < it <= 1000:
        return p_init / 16
    if 1000 < it <= 2000:
        return p_init / 32
    if 2000 < it <= 4000:
        return p_init / 64
    if 4000 < it <= 6000:
        return p_init / 128
    if 6000 < it <= 8000:
        return p_init / 256
    if 8000 < it:
        return p_init / 512
    return p_init


def margin_loss(logits, y):
    """square.py:68-86 (untargeted, loss='margin'): y_corr - max over the other classes."""
    logits = logits.clone()
    u = torch.arange(logits.shape[0])
    y_corr = logits[u, y].clone()
    logits[u, y] = -float('inf')
    return y_corr - logits.max(dim=-1)[0]


def square_linf_single_run(model_fn, x, y, eps, n_queries, p_init, rescale, init_sign, draws):
    """square.py:221-294.  init_sign: [B,c,1,w] of +-1 (random_choice); draws[i] = (vh, vw, sign[c]) of query i
    (random_int x2 + random_choice([c,1,1])).  The reference re-attacks only margin_min > 0; masks do the same."""
    with torch.no_grad():
        c, h, w = x.shape[1:]
        n_features = c * h * w
        x_best = torch.clamp(x + eps * init_sign, 0., 1.)
        margin_min = margin_loss(model_fn(x_best), y)
        loss_min = margin_min.clone()
        for i_iter in range(n_queries):
            todo = margin_min > 0.0
            if not todo.any():
                break
            p = square_p_selection(i_iter, p_init, n_queries, rescale)
            s = max(int(round(math.sqrt(p * n_features / c))), 1)
            vh, vw, sg = draws[i_iter]
            new_deltas = torch.zeros([c, h, w])
            new_deltas[:, vh:vh + s, vw:vw + s] = 2. * eps * sg.view(c, 1, 1)
            x_new = x_best + new_deltas
            x_new = torch.min(torch.max(x_new, x - eps), x + eps)
            x_new = torch.clamp(x_new, 0., 1.)
            margin = margin_loss(model_fn(x_new), y)
            loss = margin
            improved = (loss < loss_min) & todo
            loss_min = torch.where(improved, loss, loss_min)
            accept = (improved | (margin <= 0.)) & todo
            margin_min = torch.where(accept, margin, margin_min)
            x_best = torch.where(accept.view(-1, 1, 1, 1), x_new, x_best)
        return x_best


def square_linf_perturb(model_fn, x, y, eps, n_queries, p_init, rescale, init_sign_fn, draws):
    """square.py:532-600 (n_restarts = 1).  init_sign_fn(n_to_fool) supplies the start signs for the
    still-robust subset."""
    x = x.detach().clone()
    adv = x.clone()
    acc = model_fn(x).max(1)[1] == y
    ind = acc.nonzero().flatten()
    if ind.numel() != 0:
        adv_curr = square_linf_single_run(model_fn, x[ind], y[ind], eps, n_queries, p_init, rescale,
                                          init_sign_fn(ind.numel()), draws)
        fooled = (model_fn(adv_curr).max(1)[1] != y[ind]).nonzero().flatten()
        adv[ind[fooled]] = adv_curr[fooled]
    return adv


# ---------------------------------------------------------------------------------------
# Square attack, L2 and L1 (Attacks/autoattack/square.py:123-190, 296-530) -- pinned (tests/golden/square_lp_ref.npz)
# ---------------------------------------------------------------------------------------

def square_eta_rectangles(x, y, norm):
    """square.py:146-170: concentric rectangles of weight 1 / k^2 (L2) or 1 / k^4 (L1), normalised."""
    delta = torch.zeros([x, y])
    x_c, y_c = x // 2 + 1, y // 2 + 1
    c0, c1 = x_c - 1, y_c - 1
    power = 2 if norm == 'L2' else 4
    for k in range(0, max(x_c, y_c)):
        delta[max(c0, 0):min(c0 + (2 * k + 1), x), max(0, c1):min(c1 + (2 * k + 1), y)] += \
            1.0 / (torch.Tensor([k + 1]).view(1, 1) ** power)
        c0 -= 1
        c1 -= 1
    if norm == 'L2':
        delta /= (delta ** 2).sum(dim=(0, 1), keepdim=True).sqrt()
    else:
        delta /= delta.abs().sum()
    return delta


def square_eta(s, norm, transpose):
    """square.py:172-190; `transpose` is the torch.rand([1]) > 0.5 draw of :187."""
    delta = torch.zeros([s, s])
    delta[:s // 2] = square_eta_rectangles(s // 2, s, norm)
    delta[s // 2:] = -1. * square_eta_rectangles(s - s // 2, s, norm)
    if norm == 'L2':
        delta /= (delta ** 2).sum(dim=(0, 1), keepdim=True).sqrt()
    else:
        delta /= delta.abs().sum()
    return delta.permute([1, 0]) if transpose else delta


def _square_lp_norm(v, norm):
    f = v.reshape(v.shape[0], -1)
    t = (f ** 2).sum(-1).sqrt() if norm == 'L2' else f.abs().sum(dim=-1)
    return t.view(-1, 1, 1, 1)


def square_lp_single_run(model_fn, x, y, eps, n_queries, p_init, rescale, norm, draws):
    """square.py:296-530 (norm 'L2' / 'L1', loss 'margin').  draws.square_lp_init_tile(n, c) -> (transpose, signs [n, c]) per start
    tile in the reference's order; draws.square_lp_query(h, w, s, n_curr, c) -> (vh, vw, vh2, vw2, transpose, signs [n_curr, c])."""
    with torch.no_grad():
        c, h, w = x.shape[1:]
        n_features = c * h * w
        delta_init = torch.zeros_like(x)
        s = h // 5
        sp_init = (h - s * 5) // 2
        vh = sp_init
        for _ in range(h // s):
            vw = sp_init
            for _ in range(w // s):
                tr, sg = draws.square_lp_init_tile(x.shape[0], c)
                delta_init[:, :, vh:vh + s, vw:vw + s] += square_eta(s, norm, tr).view(1, 1, s, s) * sg.view(-1, c, 1, 1)
                vw += s
            vh += s
        if norm == 'L2':
            x_best = torch.clamp(x + delta_init / (_square_lp_norm(delta_init, norm) + 1e-12) * eps, 0., 1.)
        else:
            x_best = x + delta_init + l1_projection(x, delta_init, eps * (1. - 1e-6))
        margin_min = margin_loss(model_fn(x_best), y)
        loss_min = margin_min.clone()
        for i_iter in range(n_queries):
            idx = (margin_min > 0.0).nonzero().flatten()
            if idx.numel() == 0:
                break
            x_curr, x_best_curr, y_curr = x[idx], x_best[idx], y[idx]
            delta_curr = x_best_curr - x_curr
            p = square_p_selection(i_iter, p_init, n_queries, rescale)
            s = max(int(round(math.sqrt(p * n_features / c))), 3)
            if s % 2 == 0:
                s += 1
            vh, vw, vh2, vw2, tr, sg = draws.square_lp_query(h, w, s, idx.numel(), c)
            win1 = delta_curr[:, :, vh:vh + s, vw:vw + s]
            mask = torch.zeros_like(x_curr)
            mask[:, :, vh:vh + s, vw:vw + s] = 1.0
            mask[:, :, vh2:vh2 + s, vw2:vw2 + s] = 1.0
            norms_image = _square_lp_norm(x_best_curr - x_curr, norm)
            new_deltas = torch.ones([x_curr.shape[0], c, s, s]) * (square_eta(s, norm, tr).view(1, 1, s, s) * sg.view(-1, c, 1, 1))
            if norm == 'L2':
                norms_window_1 = (win1 ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()
                norms_windows = ((delta_curr * mask) ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()
                new_deltas += win1 / (1e-12 + norms_window_1)
                new_deltas = new_deltas / (1e-12 + (new_deltas ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()) * (torch.max(
                    (eps * torch.ones_like(new_deltas)) ** 2 - norms_image ** 2, torch.zeros_like(new_deltas)) / c +
                    norms_windows ** 2).sqrt()
            else:
                norms_window_1 = win1.abs().sum(dim=(-2, -1), keepdim=True)
                norms_windows = (delta_curr * mask).abs().sum(dim=(-2, -1), keepdim=True)
                new_deltas += win1 / (1e-12 + norms_window_1)
                new_deltas = new_deltas / (1e-12 + new_deltas.abs().sum(dim=(-2, -1), keepdim=True)) * (torch.max(
                    eps * torch.ones_like(norms_image) - norms_image, torch.zeros_like(norms_image)) / c + norms_windows) * c
            delta_curr[:, :, vh2:vh2 + s, vw2:vw2 + s] = 0.
            delta_curr[:, :, vh:vh + s, vw:vw + s] = new_deltas + 0
            if norm == 'L2':
                x_new = torch.clamp(x_curr + delta_curr / (_square_lp_norm(delta_curr, norm) + 1e-12) * eps, 0., 1.)
            else:
                x_new = x_curr + delta_curr + l1_projection(x_curr, delta_curr, eps * (1. - 1e-6))
            margin = margin_loss(model_fn(x_new), y_curr)
            loss = margin
            improved = (loss < loss_min[idx]).float()
            loss_min[idx] = improved * loss + (1. - improved) * loss_min[idx]
            improved = torch.max(improved, (margin <= 0.).float())
            margin_min[idx] = improved * margin + (1. - improved) * margin_min[idx]
            improved = improved.view(-1, 1, 1, 1)
            x_best[idx] = improved * x_new + (1. - improved) * x_best_curr
        return x_best


def square_lp_perturb(model_fn, x, y, eps, n_queries, p_init, rescale, norm, draws):
    """square.py:532-600 (n_restarts = 1)."""
    x = x.detach().clone()
    adv = x.clone()
    acc = model_fn(x).max(1)[1] == y
    ind = acc.nonzero().flatten()
    if ind.numel() != 0:
        adv_curr = square_lp_single_run(model_fn, x[ind], y[ind], eps, n_queries, p_init, rescale, norm, draws)
        fooled = (model_fn(adv_curr).max(1)[1] != y[ind]).nonzero().flatten()
        adv[ind[fooled]] = adv_curr[fooled]
    return adv


# ---------------------------------------------------------------------------------------
# FAB, targeted, Linf / L2 / L1 (Attacks/autoattack/fab_base.py:84-336, fab_pt.py:102-117,
# fab_projections.py:7-166) -- pinned (tests/golden/attacks_ref.npz: fabproj/*, fabproj_l2/*, fabproj_l1/*, fabt/{Linf,L2,L1}/adv)
# ---------------------------------------------------------------------------------------

def fab_projection_linf(t, w, b):
    """fab_projections.py:7-59: box-constrained Linf projection of the rows of t onto {x: w.x = b}.
    Restated with the same sort / cumsum / binary-search structure.  Returns the step d."""
    w, b = w.clone(), b.clone()
    sign = 2 * ((w * t).sum(1) - b >= 0).to(t.dtype) - 1
    w = w * sign.unsqueeze(1)
    b = b * sign
    a = (w < 0).to(t.dtype)
    nz = (w != 0).to(t.dtype)
    d = (a - t) * nz
    p = a - t * (2 * a - 1)
    indp = torch.argsort(p, dim=1)
    b = b - (w * t).sum(1)
    b0 = (w * d).sum(1)
    indp2 = indp.flip((1,))
    ws = w.gather(1, indp2)
    bs2 = -ws * d.gather(1, indp2)
    s = torch.cumsum(ws.abs(), dim=1)
    sb = torch.cumsum(bs2, dim=1) + b0.unsqueeze(1)
    n = w.shape[1]
    b2 = sb[:, -1] - s[:, -1] * p.gather(1, indp[:, 0:1]).squeeze(1)
    c_l = b - b2 > 0
    c2 = (b - b0 > 0) & (~c_l)
    lb = torch.zeros(int(c2.sum()))
    ub = torch.full_like(lb, n - 1)
    indp_, sb_, s_, p_, b_ = indp[c2], sb[c2], s[c2], p[c2], b[c2]
    for _ in range(math.ceil(math.log2(n))):
        mid = torch.floor((lb + ub) / 2)
        m2 = mid.long().unsqueeze(1)
        indcurr = indp_.gather(1, n - 1 - m2)
        bb = (sb_.gather(1, m2) - s_.gather(1, m2) * p_.gather(1, indcurr)).squeeze(1)
        c = b_ - bb > 0
        lb = torch.where(c, mid, lb)
        ub = torch.where(c, ub, mid)
    lb = lb.long()
    if c_l.any():
        lam = torch.clamp_min((b[c_l] - sb[c_l, -1]) / (-s[c_l, -1]), 0).unsqueeze(-1)
        d[c_l] = (2 * a[c_l] - 1) * lam
    u = torch.arange(int(c2.sum()))
    lam = torch.clamp_min((b[c2] - sb[c2][u, lb]) / (-s[c2][u, lb]), 0).unsqueeze(-1)
    d[c2] = torch.min(lam, d[c2]) * a[c2] + torch.max(-lam, d[c2]) * (1 - a[c2])
    return d * nz


def fab_projection_l2(t, w, b):
    """fab_projections.py:62-117: box-constrained L2 projection step.  Same sort / cumsum / binary-search structure:
    r_i = the multiplier at which coordinate i meets the box, s[k] = -F(r_(k)) with F(alpha) = sum w^2 min(alpha, r)."""
    w = w.clone()
    c = (w * t).sum(1) - b
    sign = 2 * (c >= 0).to(t.dtype) - 1
    w = w * sign.unsqueeze(1)
    c = c * sign
    live = (w.abs() > 1e-8).to(t.dtype)
    r = torch.max(t / w, (t - 1) / w).clamp(min=-1e12, max=1e12)
    r = torch.where(w.abs() < 1e-8, torch.full_like(r, 1e12), r)
    r = torch.where(r == -1e12, -r, r)
    rs, order = torch.sort(r, dim=1)
    nxt = torch.cat((rs[:, 1:], torch.zeros_like(rs[:, :1])), 1)
    rs = torch.where(rs == 1e12, torch.zeros_like(rs), rs)
    nxt = torch.where(nxt == 1e12, torch.zeros_like(nxt), nxt)
    w2s = (w ** 2).gather(1, order)
    w2tot = w2s.sum(dim=1, keepdim=True)
    tail = w2tot - torch.cumsum(w2s, dim=1)                      # slope of F after breakpoint k
    d = -(r * w) * live
    head = -w2tot * rs[:, 0:1]
    s = torch.cat((head, torch.cumsum((rs - nxt) * tail, dim=1) + head), 1)
    free = s[:, 0] + c < 0                                        # c4: no coordinate meets the box
    unreachable = (d * w).sum(dim=1) + c > 0                      # c3
    mixed = ~(free | unreachable)                                 # c2
    n = w.shape[1]
    lb = torch.zeros(int(mixed.sum()))
    ub = torch.full_like(lb, n - 1)
    s_, c_ = s[mixed], c[mixed]
    for _ in range(math.ceil(math.log2(n))):
        mid = torch.floor((lb + ub) / 2)
        above = s_.gather(1, mid.long().unsqueeze(1)).squeeze(1) + c_ > 0
        lb = torch.where(above, mid, lb)
        ub = torch.where(above, ub, mid)
    lb = lb.long()
    if free.any():
        d[free] = -(c[free] / w2tot[free].squeeze(-1)).unsqueeze(-1) * w[free]
    if mixed.any():
        u = torch.arange(int(mixed.sum()))
        tl = tail[mixed][u, lb]
        alpha = (s_[u, lb] + c_) / tl + rs[mixed][u, lb]
        alpha[tl == 0] = 0
        sat = (alpha.unsqueeze(-1) > r[mixed]).to(t.dtype)
        d[mixed] = d[mixed] * sat - alpha.unsqueeze(-1) * w[mixed] * (1 - sat)
    return d * live


def fab_projection_l1(t, w, b):
    """fab_projections.py:120-166: box-constrained L1 projection step: greedy in decreasing |w| -- the first lb coordinates go to
    their bound, coordinate number lb goes part of the way, the rest stay."""
    w = w.clone()
    c = (w * t).sum(1) - b
    sign = 2 * (c >= 0).to(t.dtype) - 1
    w = w * sign.unsqueeze(1)
    c = c * sign
    order = torch.argsort((1 / w).abs().clamp_max(1e12), dim=1)
    rank = torch.argsort(order)
    up = (w < 0).to(t.dtype)
    d = (up - t) * (w != 0).to(t.dtype)
    gains = torch.min(-w * t, w * (1 - t)).gather(1, order)       # <= 0
    s = torch.cumsum(torch.cat((c.unsqueeze(-1), gains), 1), dim=1)
    reach = s[:, -1] < 0
    lb = torch.zeros(int(reach.sum()))
    ub = torch.full_like(lb, s.shape[1])
    s_ = s[reach]
    for _ in range(math.ceil(math.log2(w.shape[1]))):
        mid = torch.floor((lb + ub) / 2)
        above = s_.gather(1, mid.long().unsqueeze(1)).squeeze(1) > 0
        lb = torch.where(above, mid, lb)
        ub = torch.where(above, ub, mid)
    lbi = lb.long()
    if reach.any():
        u = torch.arange(int(reach.sum()))
        part = order[reach][u, lbi]
        alpha = -s_[u, lbi] / w[reach][u, part]
        dr = d[reach] * (rank[reach] < lbi.unsqueeze(-1)).to(t.dtype)
        dr[u, part] = alpha
        d[reach] = dr
    return d * (w.abs() > 1e-8).to(t.dtype)


FAB_PROJECTIONS = {'Linf': fab_projection_linf, 'L2': fab_projection_l2, 'L1': fab_projection_l1}


def _fab_row_norm(v, norm):
    v = v.reshape(v.shape[0], -1)
    return v.abs().max(dim=1)[0] if norm == 'Linf' else ((v ** 2).sum(dim=1).sqrt() if norm == 'L2' else v.abs().sum(dim=1))


def fab_targeted_single_run(model_fn, x, y, target_class, eps, n_iter, alpha_max=0.1, eta=1.05, beta=0.9, norm='Linf'):
    """fab_base.py:84-270 with is_targeted=True, use_rand_start=False; norm Linf / L2 / L1."""
    project = FAB_PROJECTIONS[norm]
    x = x.detach().clone().float()
    y_pred = model_fn(x).max(1)[1]
    pred = y_pred == y
    if pred.sum() == 0:
        return x
    pred = pred.nonzero().flatten()
    la_target2 = model_fn(x).sort(dim=-1)[1][:, -target_class][pred].clone()
    im2, la2 = x[pred].clone(), y[pred].clone()
    bs = im2.shape[0]
    u1 = torch.arange(bs)
    adv = im2.clone()
    adv_c = x.clone()
    res2 = 1e10 * torch.ones([bs])
    x1 = im2.clone()
    x0 = im2.clone().reshape([bs, -1])
    for _ in range(n_iter):
        im = x1.clone().requires_grad_()
        with torch.enable_grad():
            yy = model_fn(im)
            diffy = -(yy[u1, la2] - yy[u1, la_target2])
            g, = torch.autograd.grad(diffy.sum(), im)
        with torch.no_grad():
            df = diffy.detach()
            w = g.reshape([bs, -1])
            b = -df + (g * x1).reshape(bs, -1).sum(dim=-1)
            d3 = project(torch.cat((x1.reshape([bs, -1]), x0), 0), torch.cat((w, w), 0), torch.cat((b, b), 0))
            d1, d2 = d3[:bs].reshape(x1.shape), d3[-bs:].reshape(x1.shape)
            a0 = _fab_row_norm(d3, norm).view(-1, 1, 1, 1)                                    # fab_base.py:194-203
            a0 = torch.max(a0, 1e-8 * torch.ones_like(a0))
            a1, a2 = a0[:bs], a0[-bs:]
            alpha = torch.min(torch.max(a1 / (a1 + a2), torch.zeros_like(a1)), alpha_max * torch.ones_like(a1))
            x1 = ((x1 + eta * d1) * (1 - alpha) + (im2 + d2 * eta) * alpha).clamp(0.0, 1.0)
            is_adv = model_fn(x1).max(1)[1] != la2
            if is_adv.sum() > 0:
                ia = is_adv.nonzero().flatten()
                t = _fab_row_norm(x1[ia] - im2[ia], norm)                                     # fab_base.py:226-236
                better = (t < res2[ia]).float().view(-1, 1, 1, 1)
                adv[ia] = x1[ia] * better + adv[ia] * (1 - better)
                res2[ia] = t * (t < res2[ia]).float() + res2[ia] * (t >= res2[ia]).float()
                x1[ia] = im2[ia] + (x1[ia] - im2[ia]) * beta
    ind_succ = (res2 < 1e10).nonzero().flatten()
    adv_c[pred[ind_succ]] = adv[ind_succ].clone()
    return adv_c


def fab_targeted_perturb(model_fn, x, y, eps, n_iter, n_target_classes=9, norm='Linf'):
    """fab_base.py:272-336, targeted branch, n_restarts 1."""
    adv = x.clone()
    with torch.no_grad():
        acc = model_fn(x).max(1)[1] == y
    for target_class in range(2, n_target_classes + 2):
        ind = acc.nonzero().flatten()
        if ind.numel() == 0:
            continue
        xs, ys = x[ind].clone(), y[ind].clone()
        adv_curr = fab_targeted_single_run(model_fn, xs, ys, target_class, eps, n_iter, norm=norm)
        with torch.no_grad():
            acc_curr = model_fn(adv_curr).max(1)[1] == ys
        res = _fab_row_norm(xs - adv_curr, norm)                                               # fab_base.py:296-301
        acc_curr = torch.max(acc_curr, res > eps)
        fooled = (acc_curr == 0).nonzero().flatten()
        acc[ind[fooled]] = False
        adv[ind[fooled]] = adv_curr[fooled].clone()
    return adv


def fab_single_run(model_fn, x, y, eps, n_iter, norm='Linf', target_class=None, rand_t=None, alpha_max=0.1, eta=1.05, beta=0.9):
    """FABAttack.attack_single_run (fab_base.py:84-270), general form: targeted (target_class = k-th most likely class) or UNTARGETED
    (target_class None: df / dg of every class from the full Jacobian, fab_pt.py:77-100, and per step the class whose linearised
    boundary is closest in the dual norm, fab_base.py:168-186); rand_t(shape) -> the draw `t` of a random start (use_rand_start,
    fab_base.py:133-166: Linf 2 * rand - 1, L2 / L1 randn) or None."""
    project = FAB_PROJECTIONS[norm]
    x = x.detach().clone().float()
    y_pred = model_fn(x).max(1)[1]
    pred = y_pred == y
    if pred.sum() == 0:
        return x
    pred = pred.nonzero().flatten()
    targeted = target_class is not None
    if targeted:
        la_target2 = model_fn(x).sort(dim=-1)[1][:, -target_class][pred].clone()
    im2, la2 = x[pred].clone(), y[pred].clone()
    bs = im2.shape[0]
    u1 = torch.arange(bs)
    adv = im2.clone()
    adv_c = x.clone()
    res2 = 1e10 * torch.ones([bs])
    x1 = im2.clone()
    x0 = im2.clone().reshape([bs, -1])
    if rand_t is not None:
        t = rand_t(tuple(x1.shape)).float()
        r = torch.min(res2, eps * torch.ones(res2.shape)).reshape(-1, 1, 1, 1)
        tf = t.reshape(bs, -1)
        if norm == 'Linf':
            x1 = im2 + r * t / tf.abs().max(dim=1, keepdim=True)[0].reshape(-1, 1, 1, 1) * .5
        elif norm == 'L2':
            x1 = im2 + r * t / (tf ** 2).sum(dim=-1).sqrt().view(-1, 1, 1, 1) * .5
        else:
            x1 = im2 + r * t / tf.abs().sum(dim=-1).view(-1, 1, 1, 1) / 2
        x1 = x1.clamp(0.0, 1.0)
    for _ in range(n_iter):
        im = x1.clone().requires_grad_()
        with torch.enable_grad():
            yy = model_fn(im)
            if targeted:
                diffy = -(yy[u1, la2] - yy[u1, la_target2])
                g, = torch.autograd.grad(diffy.sum(), im)
                df, dg = diffy.detach().unsqueeze(1), g.unsqueeze(1)
            else:
                g2 = torch.stack([torch.autograd.grad(yy[:, c].sum(), im, retain_graph=True)[0] for c in range(yy.shape[-1])], 1)
                y2 = yy.detach()
                df = y2 - y2[u1, la2].unsqueeze(1)
                dg = g2 - g2[u1, la2].unsqueeze(1)
                df[u1, la2] = 1e10
        with torch.no_grad():
            dgf = dg.reshape(bs, dg.shape[1], -1)
            if norm == 'Linf':
                dist1 = df.abs() / (1e-12 + dgf.abs().sum(dim=-1))
            elif norm == 'L2':
                dist1 = df.abs() / (1e-12 + (dgf ** 2).sum(dim=-1).sqrt())
            else:
                dist1 = df.abs() / (1e-12 + dgf.abs().max(dim=2)[0])
            ind = dist1.min(dim=1)[1]
            dg2 = dg[u1, ind]
            b = -df[u1, ind] + (dg2 * x1).reshape(bs, -1).sum(dim=-1)
            w = dg2.reshape([bs, -1])
            d3 = project(torch.cat((x1.reshape([bs, -1]), x0), 0), torch.cat((w, w), 0), torch.cat((b, b), 0))
            d1, d2 = d3[:bs].reshape(x1.shape), d3[-bs:].reshape(x1.shape)
            a0 = _fab_row_norm(d3, norm).view(-1, 1, 1, 1)
            a0 = torch.max(a0, 1e-8 * torch.ones_like(a0))
            a1, a2 = a0[:bs], a0[-bs:]
            alpha = torch.min(torch.max(a1 / (a1 + a2), torch.zeros_like(a1)), alpha_max * torch.ones_like(a1))
            x1 = ((x1 + eta * d1) * (1 - alpha) + (im2 + d2 * eta) * alpha).clamp(0.0, 1.0)
            is_adv = model_fn(x1).max(1)[1] != la2
            if is_adv.sum() > 0:
                ia = is_adv.nonzero().flatten()
                t = _fab_row_norm(x1[ia] - im2[ia], norm)
                better = (t < res2[ia]).float().view(-1, 1, 1, 1)
                adv[ia] = x1[ia] * better + adv[ia] * (1 - better)
                res2[ia] = t * (t < res2[ia]).float() + res2[ia] * (t >= res2[ia]).float()
                x1[ia] = im2[ia] + (x1[ia] - im2[ia]) * beta
    ind_succ = (res2 < 1e10).nonzero().flatten()
    adv_c[pred[ind_succ]] = adv[ind_succ].clone()
    return adv_c


def fab_perturb(model_fn, x, y, eps, n_iter, n_restarts=1, norm='Linf', targeted=False, n_target_classes=9, start_draw=None):
    """FABAttack.perturb (fab_base.py:272-336) with restarts: restart 0 starts at the clean point, every later one at a random point
    (start_draw(norm, shape) -> t, drawn from the torch stream the caller re-seeded like perturb() does, fab_base.py:281).  Untargeted:
    the `fab` stage of AutoAttack version 'plus' (autoattack.py:269-270); targeted with n_restarts > 1: its `fab-t` stage."""
    adv = x.clone()
    with torch.no_grad():
        acc = model_fn(x).max(1)[1] == y
    rounds = [None] if not targeted else list(range(2, n_target_classes + 2))
    for target_class in rounds:
        for counter in range(n_restarts):
            ind = acc.nonzero().flatten()
            if ind.numel() == 0:
                continue
            xs, ys = x[ind].clone(), y[ind].clone()
            rt = (lambda shape: start_draw(norm, shape)) if counter > 0 else None
            adv_curr = fab_single_run(model_fn, xs, ys, eps, n_iter, norm, target_class, rt)
            with torch.no_grad():
                acc_curr = model_fn(adv_curr).max(1)[1] == ys
            res = _fab_row_norm(xs - adv_curr, norm)
            acc_curr = torch.max(acc_curr, res > eps)
            fooled = (acc_curr == 0).nonzero().flatten()
            acc[ind[fooled]] = False
            adv[ind[fooled]] = adv_curr[fooled].clone()
    return adv


def fab_start_draw(norm, shape):
    """the `t` of FAB's random start from torch's global generator (fab_base.py:134, :143, :154)"""
    return 2 * torch.rand(tuple(shape)) - 1 if norm == 'Linf' else torch.randn(tuple(shape))


# ---------------------------------------------------------------------------------------
# AutoAttack orchestrator, Linf (Attacks/autoattack/autoattack.py:90-211) -- pinned
# ---------------------------------------------------------------------------------------

class TorchStreamDraws:
    """The random draws of the reference's sub-attacks, made from torch's GLOBAL generator in the reference's order
    (each attack's perturb() re-seeds it first: autopgd_base.py:502, :644, square.py:567, fab_base.py:281):
      APGD / APGD-T start direction  2 * rand(x.shape) - 1           (autopgd_base.py:214)
      Square start signs             sign(2 * rand([n, c, 1, w]) - 1) (square.py:114,246)
      Square query i                 randint h, randint w, sign(2 * rand([c, 1, 1]) - 1)   (square.py:118,268-274)"""

    def __init__(self, seed):
        self.seed = seed

    def reseed(self):
        torch.random.manual_seed(self.seed)

    def pm1(self, _index, shape):
        return 2 * torch.rand(tuple(shape)) - 1

    def randn(self, _index, shape):                      # APGD-L1 start (autopgd_base.py:223, :538)
        return torch.randn(tuple(shape))

    def fab_start(self, norm, shape):                    # FAB restarts > 0 (fab_base.py:134, :143, :154)
        return fab_start_draw(norm, shape)

    def square_init(self, n, c, w):
        return torch.sign(2 * torch.rand([n, c, 1, w]) - 1)

    def square_lp_init_tile(self, n, c):                 # eta(): rand([1]) > 0.5 (square.py:187), then random_choice([n, c, 1, 1]) (:304-306)
        tr = bool(torch.rand([1]) > 0.5)
        return tr, torch.sign(2 * torch.rand([n, c, 1, 1]) - 1).view(n, c)

    def square_lp_query(self, h, w, s, n_curr, c):       # square.py:333-355: four random_int, eta's transposition, the signs
        vh = int((0 + (h - s) * torch.rand([1])).long())
        vw = int((0 + (w - s) * torch.rand([1])).long())
        vh2 = int((0 + (h - s) * torch.rand([1])).long())
        vw2 = int((0 + (w - s) * torch.rand([1])).long())
        tr = bool(torch.rand([1]) > 0.5)
        return vh, vw, vh2, vw2, tr, torch.sign(2 * torch.rand([n_curr, c, 1, 1]) - 1).view(n_curr, c)

    def square_draws(self, c, h, w, n_queries, p_init=0.8, rescale=False):
        outer = self

        class _Draws:
            def __getitem__(self, i):
                p = square_p_selection(i, p_init, n_queries, rescale)
                s = max(int(round(math.sqrt(p * h * w))), 1)
                vh = int((0 + (h - s) * torch.rand([1])).long())
                vw = int((0 + (w - s) * torch.rand([1])).long())
                return vh, vw, torch.sign(2 * torch.rand([c, 1, 1]) - 1).view(c)
        del outer
        return _Draws()


def autoattack_linf(model_fn, x_orig, y_orig, eps, draws, plan=('apgd-ce', 'apgd-t', 'fab-t', 'square'), apgd_iter=100,
                    apgdt_iter=100, apgdt_classes=9, fab_iter=100, fab_classes=9, square_queries=5000, trace=None, norm='Linf', eot_iter=1):
    """AutoAttack.run_standard_evaluation (autoattack.py:90-211) with bs >= len(x), version 'standard' hyper-parameters
    (autoattack.py:253-267) unless overridden.  model_fn takes x in [0,1] (NormalizeModel already applied).
    draws: a TorchStreamDraws-like object; trace (list) receives (attack, robust_flags copy) after every attack."""
    with torch.no_grad():
        robust = y_orig.eq(model_fn(x_orig).max(1)[1])                      # :95-109
        x_adv = x_orig.clone().detach()
        c, h, w = x_orig.shape[1:]
        for attack in plan:
            if int(robust.sum()) == 0:                                       # :117-121
                break
            idcs = robust.nonzero().flatten()                                # :125-135
            x, y = x_orig[idcs].clone(), y_orig[idcs].clone()
            draws.reseed()                                                   # each perturb() re-seeds with the same seed
            start = draws.randn if norm == 'L2' else draws.pm1              # autopgd_base.py:214-221 (norm 'Linf' / 'L2' here)
            with torch.enable_grad():
                if attack in ('apgd-ce', 'apgd-dlr'):                        # (version 'rand': both, with eot_iter passes per gradient)
                    adv_curr = apgd_perturb(model_fn, x, y, norm, eps, apgd_iter, attack[5:], start, 1, eot_iter)
                elif attack == 'apgd-t':
                    adv_curr = apgd_targeted_perturb(model_fn, x, y, norm, eps, apgdt_iter, start, apgdt_classes)
                elif attack == 'fab-t':
                    adv_curr = fab_targeted_perturb(model_fn, x, y, eps, fab_iter, fab_classes, norm=norm)
                elif attack == 'square' and norm != 'Linf':
                    adv_curr = square_lp_perturb(model_fn, x, y, eps, square_queries, 0.8, False, norm, draws)
                elif attack == 'square':
                    adv_curr = square_linf_perturb(model_fn, x, y, eps, square_queries, 0.8, False,
                                                   lambda n: draws.square_init(n, c, w),
                                                   draws.square_draws(c, h, w, square_queries))
                else:
                    raise ValueError('Attack not supported')
            false_batch = ~y.eq(model_fn(adv_curr).max(1)[1])                # :179-184
            non_robust = idcs[false_batch]
            robust[non_robust] = False
            x_adv[non_robust] = adv_curr[false_batch].detach()
            if trace is not None:
                trace.append((attack, robust.clone()))
    return x_adv


def pgd_l1_art(loss_grad, x, y, eps, eps_step, max_iter, init_signed_exp, init_radius):
    """ART ProjectedGradientDescentPyTorch(norm=1, num_random_init=1), the attack behind the reference's `pgd_l1`
    (RobustART/noise/utils/adv/attack.py:44-49).  PARITY UNPINNED: ART is an unvendored, version-unpinned dependency
    (requirements.txt:25) absent from this container; this restates the published ART 1.x algorithm
    (attacks/evasion/projected_gradient_descent/projected_gradient_descent_pytorch.py: _compute_perturbation_pytorch,
    _apply_perturbation_pytorch, _projection; utils.random_sphere).  fp32 op by op.

    loss_grad(x, y) -> d CE / dx (any positive per-sample scale: the step normalises by the L1 norm);
    init_signed_exp [B, n]: sign_i * e_i with e ~ Exp(1) (normalised spacings = ART's sorted-uniform spacings in
    distribution); init_radius [B]: sqrt(U(0, eps^2))."""
    import numpy as np
    f32 = np.float32
    tol = f32(10e-8)
    B = x.shape[0]
    x0 = x.astype(f32)
    se = init_signed_exp.astype(f32).reshape(B, -1)
    ssum = np.zeros(B, f32)
    for b in range(B):
        ssum[b] = np.abs(se[b]).astype(np.float64).sum()            # the kernel sums in a fixed 2-level order (fp32)
    xa = np.clip(x0 + (se * (init_radius.astype(f32) / ssum)[:, None]).reshape(x0.shape), f32(0), f32(1)).astype(f32)
    for _ in range(max_iter):
        g = loss_grad(xa, y).astype(f32).reshape(B, -1)
        gn = np.abs(g).astype(np.float64).sum(1).astype(f32) + tol
        step = (f32(eps_step) * (g / gn[:, None])).reshape(x0.shape)
        xa = np.clip(xa + step, f32(0), f32(1)).astype(f32)
        d = (xa - x0).reshape(B, -1)
        fac = np.minimum(f32(1.0), f32(eps) / (np.abs(d).astype(np.float64).sum(1).astype(f32) + tol))
        xa = (d * fac[:, None]).reshape(x0.shape) + x0
    return xa.astype(f32)
