"""Renorm ('dr') under sync-WC with TWO real ranks (the launcher of tests/test_sync_wc_two_ranks_gpu.py: two processes share cuda:0 and meet
over gloo, each with its own half of the batch).  The batch factor L comes from the all-reduced moments, so on BOTH ranks the value is
the moving-statistics whitening of the global batch, W_m (x - mu_global) Gamma + beta, and dx is the global batch's: the float64 oracle's
renorm (oracle.wc_oracle.wc_forward_renorm / wc_backward_renorm) on the concatenation, 1e-4 relative max-norm.  (A route that factors the
LOCAL moments for C0 and whitens with the global W -- C0 W_batch != W_m -- fails this.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RANK = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r)
rank, rdzv, out = int(sys.argv[1]), sys.argv[2], sys.argv[3]
dist.init_process_group("gloo", init_method="file://" + rdzv, rank=rank, world_size=2)
from wc_gan_amd.functional import whiten_color
d = np.load(out + "/inputs.npz")
n = d["x"].shape[0] // 2
lo, hi = (0, n) if rank == 0 else (n, 2 * n)
dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")
C = d["x"].shape[-1]
x = dev(d["x"][lo:hi]).requires_grad_(True)
G, B = dev(d["G"]).requires_grad_(True), dev(d["B"]).requires_grad_(True)
mm, mc = dev(d["mm"]).view(C, 1), dev(d["mc"])
y = whiten_color(x, G, B, None, mm, mc, True, process_group=dist.group.WORLD, renorm=True)
y.backward(dev(d["gy"][lo:hi]))
torch.cuda.synchronize()
np.savez(out + "/rank%%d.npz" %% rank, y=y.detach().cpu().numpy(), dx=x.grad.cpu().numpy(), dG=G.grad.cpu().numpy(), dB=B.grad.cpu().numpy(),
         mc=mc.cpu().numpy())
dist.barrier()
dist.destroy_process_group()
''' % ROOT


def test_renorm_under_sync_wc_is_the_moving_whitening_of_the_global_batch(tmp_path):
    from oracle import wc_oracle as o
    rng = np.random.default_rng(23)
    shape = (8, 4, 4, 64)
    C = shape[-1]
    # the two halves differ in scale and offset: local and global batch statistics are far apart
    x = o.synth_activation(rng, shape, "well")
    x[:4] = 1.6 * x[:4] + 0.4
    x[4:] = 0.7 * x[4:] - 0.3
    x = x.astype(np.float32)
    mm, mc = o.moments_to_stats(*o.batch_moments(1.2 * o.synth_activation(rng, (40 * C, C), "well") + 0.05))
    mm, mc = mm.astype(np.float32), mc.astype(np.float32)
    G, B = o.synth_coloring(rng, C, 1)
    G, B = G.astype(np.float32), B.astype(np.float32)
    gy = rng.standard_normal(shape).astype(np.float32)
    np.savez(tmp_path / "inputs.npz", x=x, G=G, B=B, gy=gy, mm=mm, mc=mc)
    env = dict(os.environ, WC_K2_TWO_LAUNCH="1")          # two processes time-slice one GPU: the K2 form without an in-launch wait
    procs = [subprocess.Popen([sys.executable, "-c", RANK, str(r), str(tmp_path / "rdzv"), str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o_[-1500:] for o_ in outs)
    y_ref, cache = o.wc_forward_renorm(x, G, B, None, moving_mean=mm.astype(np.float64), moving_cov=mc.astype(np.float64))
    dx_ref, dG_ref, dB_ref = o.wc_backward_renorm(gy, cache)
    # the documented property itself: the value is W_m (x - mu_global) Gamma + beta
    X = x.reshape(-1, C).astype(np.float64)
    Wm = o.whitening_matrix(mc.astype(np.float64))[1]
    direct = ((X - X.mean(0)) @ Wm.T @ G[0].astype(np.float64) + B[0]).reshape(shape)
    assert np.abs(direct - y_ref).max() <= 1e-10 * np.abs(y_ref).max()
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(np.asarray(b)).max(), 1e-30))
    cat = lambda k: np.concatenate([r0[k], r1[k]], axis=0)
    errs = dict(y0=rel(r0["y"], y_ref[:4]), y1=rel(r1["y"], y_ref[4:]), y=rel(cat("y"), y_ref), dx=rel(cat("dx"), dx_ref),
                dG=rel(r0["dG"] + r1["dG"], dG_ref), dB=rel(r0["dB"] + r1["dB"], dB_ref),
                mc0=rel(r0["mc"], cache['moving_cov']), mc1=rel(r1["mc"], cache['moving_cov']))
    print(errs)
    assert all(v < 1e-4 for v in errs.values()), errs
