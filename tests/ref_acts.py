"""The three rectifiers with curvature (leaky ReLU, ELU, softplus) for the torch reference, and the
engine's act' and act'' through the post-activation value y as numpy functions. CPU only.

Importing this module adds the three entries to ref_mlp.ACTS, so net_out, loss_grad, gn_ref, hess_ref, grad_sq_ref
and hf_ref take the new names as they are. The forms pass through jvp, vjp, vmap(grad), jacrev and
autograd.functional.hvp. softplus is logaddexp(z, 0), not F.softplus: that one is the identity above its threshold
of 20. ELU's expm1 sees clamp(z, max=0), so the branch torch.where discards never overflows into its gradient.
"""
import numpy as np
import torch

import ref_mlp

NEW_ACTS = ["leaky_relu", "elu", "softplus"]
LEAKY_SLOPE = 0.01

ref_mlp.ACTS.update({
    "leaky_relu": lambda z: torch.where(z > 0, z, LEAKY_SLOPE * z),
    "elu": lambda z: torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0))),
    "softplus": lambda z: torch.logaddexp(z, torch.zeros_like(z)),
})


def act(name, x):
    """act(x) in the dtype of the array x (fp64 for the references)."""
    return ref_mlp.ACTS[name](torch.as_tensor(np.asarray(x))).numpy()


def dact_y(name, y):
    """act' as a function of y = act(x)."""
    y = np.asarray(y, np.float64)
    if name == "leaky_relu":
        return np.where(y > 0, 1.0, LEAKY_SLOPE)
    if name == "elu":
        return np.where(y > 0, 1.0, y + 1.0)
    if name == "softplus":
        return -np.expm1(-y)
    raise KeyError(name)


def d2act_y(name, y):
    """act'' as a function of y = act(x)."""
    y = np.asarray(y, np.float64)
    if name == "leaky_relu":
        return np.zeros_like(y)
    if name == "elu":
        return np.where(y > 0, 0.0, y + 1.0)
    if name == "softplus":
        return np.exp(-y) * -np.expm1(-y)
    raise KeyError(name)
