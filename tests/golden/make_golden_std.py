"""Writes tests/golden/std_golden.npz from tests/std_reference.py: one small conditional site, every mode the reference has.
Run from the repository root:  python tests/golden/make_golden_std.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import std_reference as R  # noqa: E402


def cases():
    rng = np.random.default_rng(20190506)
    N, H, W, C, K = 6, 3, 3, 32, 3
    x = (rng.standard_normal((N, H, W, C)) * 10.0 ** rng.uniform(-2, 1, C) + 3.0 * rng.standard_normal(C)).astype(np.float32)
    gamma = (1.0 + 0.5 * rng.standard_normal((K, C))).astype(np.float32)
    beta = (0.3 * rng.standard_normal((K, C))).astype(np.float32)
    slot = rng.integers(0, K, N).astype(np.int32)
    gy = rng.standard_normal((N, H, W, C)).astype(np.float32)
    mm = (0.1 * rng.standard_normal(C)).astype(np.float32)
    mv = (1.0 + 0.2 * rng.random(C)).astype(np.float32)
    out = dict(x=x, gamma=gamma, beta=beta, slot=slot, gy=gy, moving_mean=mm, moving_variance=mv)
    for relu in (0, 1):
        for ddof in (0, 1):
            y, c = R.forward(x, gamma, beta, slot, mm, mv, True, 1e-3, 0.99, ddof, bool(relu))
            dx, dg, db = R.backward(gy, c)
            tag = f"train_relu{relu}_ddof{ddof}"
            out.update({f"{tag}_y": y, f"{tag}_dx": dx, f"{tag}_dgamma": dg, f"{tag}_dbeta": db, f"{tag}_mu": c['mu'], f"{tag}_w": c['w'],
                        f"{tag}_moving_mean": c['moving_mean'], f"{tag}_moving_variance": c['moving_variance']})
    y, c = R.forward(x, gamma, beta, slot, mm, mv, False, relu=True)
    dx, dg, db = R.backward(gy, c)
    out.update(eval_y=y, eval_dx=dx, eval_dgamma=dg, eval_dbeta=db)
    y, c = R.forward(x, gamma, beta, slot, mm, mv, True, ddof=0, relu=True, groups=3)
    out.update(groups3_y=y, groups3_mu=c['mu'], groups3_w=c['w'], groups3_moving_mean=c['moving_mean'],
               groups3_moving_variance=c['moving_variance'])
    y, c = R.forward(x, None, None, None, mm, mv, True)
    out.update(plain_y=y, plain_dx=R.backward(gy, c)[0])
    return out


if __name__ == "__main__":
    np.savez(os.path.join(HERE, "std_golden.npz"), **cases())
