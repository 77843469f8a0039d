"""The blocked SOR's launch-range case, shared by the SOR and pool-content tests."""
import torch

from hnanosolver_amd import device as D


def range_sweep(part, div, p0, iters, first, count, dx, omega, what):
    """`iters` iterations of D.rbgs_iterate on `part`, a grid whose launch range is [first, first + count), from p0 in p_a and 7.0 in p_b (stale content of the second
    buffer must not matter). Only the leaves of the range may be stored: outside it both buffers keep what they held. -> (the result buffer, p_a, p_b, the range's slice)"""
    p_a, p_b = p0.clone(), torch.full_like(p0, 7.0)
    out = D.rbgs_iterate(part, div, p_a, p_b, dx, omega, iters)
    sl = slice(first * 512, (first + count) * 512)
    keep = torch.ones(p0.numel(), dtype=torch.bool, device=p0.device)
    keep[sl] = False
    assert bool((p_b[keep] == 7.0).all()), f"{what}: a leaf outside the range was written"
    assert torch.equal(p_a[keep].view(torch.int32), p0[keep].view(torch.int32)), f"{what}: a leaf outside the range was written in the first buffer"
    return out, p_a, p_b, sl
