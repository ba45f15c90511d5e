"""Development: is one WGAN-GP critic update (train.WGAN_CONFIGS, batch 8 + 8) reproducible bit for bit?  The same update -- same seeds,
same inputs, a fresh trainer each time -- three times on the separate autograd nodes (conv.FUSED_BLOCK = False, the route before the
critic block became one node) and twice on the one node, every pair compared: loss, penalty, the gradients handed to the optimizer and
the split records of every site.  The answer on an MI355X: loss and penalty reproduce, 11 gradients and the penalty's 't' records do
not, on either route and between two runs of the same route alike.
usage: wgan_update_repro.py      -> profiles/critic_glue_wgan_repro.txt"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch
from test_critic_glue_gpu import _wgan_update


def main():
    runs = [('separate0', False), ('separate1', False), ('fused0', True), ('separate2', False), ('fused1', True)]
    res = {name: _wgan_update(fused) for name, fused in runs}
    names = [r[0] for r in runs]
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            (la, wa, ra, pa, _, fa), (lb, wb, rb, pb, _, fb) = res[a], res[b]
            w = [n for n in wa if not torch.equal(wa[n], wb[n])]
            d = {n: float((fa[n] - fb[n]).abs().max() / fa[n].abs().max()) for n in fa if not torch.equal(fa[n], fb[n])}
            r = sorted({k[2] for k in ra if not torch.equal(ra[k], rb[k])})
            print(f"{a} vs {b}: loss equal {bool(torch.equal(la, lb))}, penalty equal {bool(torch.equal(pa, pb))}, Wasserstein-pass "
                  f"gradients that differ {len(w)}, final gradients that differ {len(d)} (worst {max(d.values(), default=0.0):.2e} of the "
                  f"tensor's maximum), record roles that differ {r}", flush=True)


if __name__ == '__main__':
    main()
