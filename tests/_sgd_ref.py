"""The SGD rule of ``mc_sgd_step`` (include/mammoclip_hip.h) restated on the CPU with ONE torch operation per rounding: every
product is a ``torch.mul`` of fp32 tensors, every sum a ``torch.add`` / ``torch.sub`` without ``alpha``.  The hyper-parameters
are rounded to fp32 once (``f32``), as the entry point does on the host.  Shared by test_sgd.py and test_sgd_gpu.py, which
compare the kernel with it on bits; test_sgd.py ties it to ``torch.optim.SGD`` in float64 with a bound counted from the rule.

Also here: that bound (``fp64_step`` returns the float64 values together with the same expressions over absolute values)."""
import torch

U = 2.0 ** -24                     # unit round-off of fp32
K_BUF, K_P = 6, 10                 # fp32 roundings on the path to buf and to p, counted from the rule


def f32(x):
    """a python float rounded to fp32 once, as a 0-dim fp32 tensor"""
    return torch.tensor(float(x), dtype=torch.float64).to(torch.float32)


def ema_weight(k, decay, warmup=True):
    """w of the k-th applied EMA update: double arithmetic, one rounding to fp32"""
    d = min(decay, (1.0 + k) / (10.0 + k)) if warmup else decay
    return torch.tensor(1.0 - d, dtype=torch.float64).to(torch.float32)


def ema_update(e, p, w):
    """e + w * (p - e): sub, mul, add"""
    return torch.add(e, torch.mul(torch.sub(p, e), w))


def sgd_step(p, g, buf, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False, coef=None):
    """one APPLIED step on fp32 CPU tensors.  ``buf`` None: the first applied step of this tensor (buf = g').  ``coef``: the clip
    coefficient, an fp32 tensor.  Returns (p, buf); buf stays None when momentum == 0.  Nothing is modified in place."""
    assert p.dtype == g.dtype == torch.float32
    g = torch.neg(g) if maximize else g
    if coef is not None:
        g = torch.mul(g, coef.detach().cpu().to(torch.float32).reshape(()))
    if weight_decay != 0:
        g = torch.add(g, torch.mul(p, f32(weight_decay)))
    if momentum != 0:
        if buf is None:
            buf = g.clone()
        else:
            buf = torch.add(torch.mul(buf, f32(momentum)), torch.mul(g, f32(1.0 - dampening)))
        d = torch.add(g, torch.mul(buf, f32(momentum))) if nesterov else buf
    else:
        d, buf = g, None
    return torch.sub(p, torch.mul(d, f32(lr))), buf


class Replay:
    """the optimizer over a list of tensors, with the skipped-step behaviour of the loss-scaled step and the EMA line:
    ``step(grads, skipped=True)`` changes nothing at all (no buffer appears, the EMA count stays); a ``None`` gradient leaves that
    tensor out of the step, and its first step is its own."""

    def __init__(self, params, shadows=None, decay=0.9, warmup=True, **hyper):
        self.p = [t.detach().cpu().clone() for t in params]
        self.buf = [None] * len(self.p)
        self.e = [t.detach().cpu().clone() for t in shadows] if shadows is not None else None
        self.decay, self.warmup, self.updates, self.hyper = decay, warmup, 0, hyper

    def step(self, grads, coef=None, skipped=False):
        if skipped:
            return
        w = ema_weight(self.updates + 1, self.decay, self.warmup) if self.e is not None else None
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.p[i], self.buf[i] = sgd_step(self.p[i], g.detach().cpu(), self.buf[i], coef=coef, **self.hyper)
            if w is not None:
                self.e[i] = ema_update(self.e[i], self.p[i], w)
        self.updates += 1


def fp64_step(p, g, buf, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False):
    """the same step in float64 on the same fp32-valued inputs (hyper-parameters as the fp32 values the kernel uses), and next
    to every value the expression with every term replaced by its absolute value: -> (p, buf, A_p, A_buf).
    |x32 - x64| <= k * 2^-24 * A * 1.01 with k = K_BUF for buf and K_P for p: each of the k roundings on the path contributes at most
    2^-24 times a partial result, every partial result is bounded by A, and the 1.01 covers the second-order terms
    ((1 + 2^-24)^10 - 1 = 10 * 2^-24 * (1 + 3e-7))."""
    lr, mu, omd, wd = (float(f32(x)) for x in (lr, momentum, 1.0 - dampening, weight_decay))
    p, g = p.double(), g.double()
    g = -g if maximize else g
    a_g = g.abs()
    if weight_decay != 0:
        g, a_g = g + wd * p, a_g + wd * p.abs()
    if momentum != 0:
        if buf is None:
            buf, a_buf = g.clone(), a_g.clone()
        else:
            buf, a_buf = mu * buf.double() + omd * g, mu * buf.double().abs() + omd * a_g
        d, a_d = (g + mu * buf, a_g + mu * a_buf) if nesterov else (buf, a_buf)
    else:
        d, a_d, buf, a_buf = g, a_g, None, None
    return p - lr * d, buf, p.abs() + lr * a_d, a_buf


def combos():
    """every (momentum, dampening, nesterov, weight_decay, maximize) torch.optim.SGD accepts out of
    {0, 0.9} x {0, 0.5} x {F, T} x {0, 1e-2} x {F, T}"""
    out = []
    for mu in (0.0, 0.9):
        for damp in (0.0, 0.5):
            for nest in (False, True):
                if nest and (mu <= 0 or damp != 0):
                    continue
                for wd in (0.0, 1e-2):
                    for mx in (False, True):
                        out.append(dict(momentum=mu, dampening=damp, nesterov=nest, weight_decay=wd, maximize=mx))
    return out
