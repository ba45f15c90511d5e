"""A float64 numpy Adam with the recipes' learning-rate schedules, written from the textbook form (Kingma & Ba, algorithm 1, with the
bias-corrected moments spelt out) and the schedule table of the reference's run.py:99-144 -- independently of wc_gan_amd/optim.py, which
folds the corrections into two scalars.  Not collected: no test_ prefix.

`it` counts the updates already applied: the first update runs at multiplier 1."""
import numpy as np


def multiplier(kind, it, total=None, ratio=1):
    if kind is None:
        return 1.0
    it = float(it)
    decayed = 1.0 - it / total
    if decayed < 0.0:
        decayed = 0.0
    if kind == 'linear':
        return decayed
    if kind == 'half-linear':
        return decayed if 2.0 * it < total else 0.5
    if kind == 'linear-end':
        knee = 0.828 * total
        if it <= knee:
            return 1.0
        left = 1.0 - (it - knee) / (total - knee)
        return left if left > 0.0 else 0.0
    assert kind.startswith('dropat'), kind
    drop = int(kind[len('dropat'):]) * 1000 * ratio
    return decayed * (1.0 if it < drop else 0.1)


class Adam64:
    """params: a list of float64 arrays (copied).  step(grads): one update; a None gradient skips that parameter (its moments stay, it
    shares the one counter)."""

    def __init__(self, params, lr, betas, eps=1e-8, schedule=None, total_iters=None, ratio=1):
        self.p = [np.array(p, dtype=np.float64) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.lr, (self.b1, self.b2), self.eps = lr, betas, eps
        self.schedule, self.total, self.ratio = schedule, total_iters, ratio
        self.t = 0

    def rate(self):
        return self.lr * multiplier(self.schedule, self.t, self.total, self.ratio)

    def step(self, grads):
        rate = self.rate()
        self.t += 1
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = np.asarray(g, dtype=np.float64)
            self.m[i] = self.b1 * self.m[i] + (1.0 - self.b1) * g
            self.v[i] = self.b2 * self.v[i] + (1.0 - self.b2) * g * g
            m_hat = self.m[i] / (1.0 - self.b1 ** self.t)
            v_hat = self.v[i] / (1.0 - self.b2 ** self.t)
            self.p[i] = self.p[i] - rate * m_hat / (np.sqrt(v_hat) + self.eps)
