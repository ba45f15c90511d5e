"""Float64 references of the gradient penalty  P = weight * mean_n (||grad_x D(x_n)|| - 1)^2  by torch's own double backward; plain torch,
any device, not collected.

`module_penalty`: through a wc_gan_amd Discriminator module run by torch ops (CPU float64: every layer is differentiable twice there).
`reference_penalty`: through tests/critic_reference.Critic built from a state dict, optionally with forced ReLU masks -- the form the GPU
tests use, where an fp32 network and a float64 one disagree on signs within rounding of zero.
Both return (penalty, norms, {parameter name: gradient}); a parameter the penalty does not reach has a zero gradient.
"""
import torch

import critic_reference as R


def _penalty(out, x, weight, params):
    out = out[0] if isinstance(out, tuple) else out
    g, = torch.autograd.grad(out.sum(), x, create_graph=True)
    norms = g.flatten(1).norm(dim=1)
    pen = weight * ((norms - 1) ** 2).mean()
    grads = torch.autograd.grad(pen, params, allow_unused=True)
    return pen.detach(), norms.detach(), [torch.zeros_like(p) if g is None else g.detach() for p, g in zip(params, grads)]


def module_penalty(D, x, cls, weight):
    x = x.detach().clone().requires_grad_(True)
    names, params = zip(*D.named_parameters())
    pen, norms, grads = _penalty(D(x, cls), x, weight, params)
    return pen, norms, dict(zip(names, grads))


def reference_penalty(state, kw, x, cls, weight, masks=None):
    """-> (penalty, norms, gradients, the Critic: its .pre holds the float64 pre-activations for critic_reference.mask_disagreement)"""
    params, buffers = R.leaves(state)
    critic = R.Critic(params, buffers, iterations=0, masks=masks, **kw)
    x64 = x.detach().double().clone().requires_grad_(True)
    names = list(params)
    pen, norms, grads = _penalty(critic(x64, cls), x64, weight, [params[n] for n in names])
    return pen, norms, dict(zip(names, grads)), critic


def rel(a, ref):
    """max |a - ref| over the tensor's maximum (an all-zero reference: the absolute error)"""
    scale = float(ref.detach().abs().max())
    return float((a.detach().double() - ref.detach().double()).abs().max()) / (scale if scale > 0 else 1.0)
