"""Device-side plumbing shared by the GPU tests: host arrays to the device and back, a case of ref_mlp.make_case as the
arguments of the engine's calls, and the in-process rank group. The references these are compared with live in
ref_mlp.py."""
import threading

import numpy as np
import torch


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.double().cpu().numpy()


def gpu_args(c):
    """(P, b, X, Y, idx) of a case on the device; idx is None unless the case gathers its rows."""
    gathered = len(c["rows"]) != len(c["X"])
    idx = torch.from_numpy(c["rows"].astype(np.int32)).cuda() if gathered else None
    return dev(c["P"]), dev(c["b"]), dev(c["X"]), dev(c["Y"]), idx


def make_net(pkg, ctx, c, l2=0.0):
    return pkg.Mlp(ctx, c["dims"], c["acts"], loss=c["loss"], l2=l2)


def solver_inputs(c):
    """The batch rows of the case, no gather: (P, X, Y) on the device (P a fresh copy: the solver updates it)."""
    return dev(c["P"]), dev(c["X"][c["rows"]]), dev(c["Y"][c["rows"]])


def run_ranks(pkg, world, body, timeout=240):
    """body(rank, ctx) on `world` threads, each a rank of one in-process group (lbf_comm_init_local) on GPU 0.
    Returns the per-rank results; re-raises the first rank exception."""
    ctxs = [pkg.Context(0, use_torch_stream=False) for _ in range(world)]
    pkg.Context.comm_init_local(ctxs)
    torch.cuda.synchronize()
    out, err = [None] * world, [None] * world

    def th(r):
        try:
            torch.cuda.set_device(0)
            out[r] = body(r, ctxs[r])
            torch.cuda.synchronize()
        except BaseException as e:  # noqa: BLE001 (re-raised below)
            err[r] = e

    ts = [threading.Thread(target=th, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
    assert not any(t.is_alive() for t in ts), "a rank thread did not finish"
    for e in err:
        if e is not None:
            raise e
    return out


def shard(N, world, r):
    return N * r // world, N * (r + 1) // world
