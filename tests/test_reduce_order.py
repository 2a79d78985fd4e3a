"""The order of additions of the fixed-order reductions (rag_amd/csrc/reduce.h), pinned at the one place where the whole arithmetic
can be restated exactly on the CPU: the gradient norm of ragmi_sgd_clip_step.  The kernel squares floats in double (exact: 24 + 24
bits) and adds them in double
  - per thread, grid-stride over 256 workgroups x 256 threads (element i of trip t belongs to workgroup (i / 256) % 256, thread i % 256),
  - over the 64 lanes of each wave by xor butterflies 32, 16, ... 1,
  - over the four waves as (w0 + w1) + (w2 + w3),
then every workgroup of the update launch adds the 256 partials the same way (thread t holds partial t) and the norm is
float(sqrt(total)).  `restate` below is that, in numpy.  The CPU test shows that it sums every element exactly once; the GPU test
that the kernel's norm equals it bit for bit."""
import math

import numpy as np
import pytest
import torch

SIZES = (1, 63, 257, 65537, 2 * 65536 + 17)     # one lane; a partial wave; a second workgroup; thread 0's second trip only; three trips
WG = 256                                         # threads per workgroup = workgroups = partials (SGD_PARTS)


def gradient(n):
    """N(0, 1) with one row of 64 scaled by 2^20.  From n = 257 on the row is a part of the elements and the sum of such squares
    depends on the order of additions; at n = 1 and n = 63 the row is everything (a common factor), and those sizes check the
    lanes that hold no element, not the order."""
    g = np.random.RandomState(n).randn(n).astype(np.float32)
    r = (n // 64) // 2
    g[64 * r:64 * (r + 1)] *= np.float32(2.0 ** 20)
    return g


def squares(g, active=None):
    sq = g.astype(np.float64) ** 2              # exact
    return sq if active is None else sq * active.astype(np.float64)      # an inactive element adds an exact +0.0


def block_wave_sum(v):
    """v[..., 256] -> [...]: butterflies within each wave of 64, then (w0 + w1) + (w2 + w3)"""
    s = v.reshape(v.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    w = s[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def restate(sq):
    """the kernels' total of the squares `sq`, in their order"""
    trips = -(-sq.size // (WG * WG))
    padded = np.zeros(trips * WG * WG, np.float64)         # past the end a thread adds nothing; + 0.0 leaves a sum >= +0.0 as it is
    padded[:sq.size] = sq
    s = np.zeros((WG, WG), np.float64)                     # [workgroup][thread]
    for t in padded.reshape(trips, WG, WG):
        s = s + t
    part = block_wave_sum(s)                               # [workgroup]
    return float(block_wave_sum(part))


def norm_bits(total):
    return int(np.float32(np.sqrt(np.float64(total))).view(np.uint32))


@pytest.mark.parametrize("n", SIZES)
def test_restatement_sums_every_element_once(n):
    """every element reaches the total through trips + 6 + 2 additions in its workgroup and 6 + 2 among the partials, all of
    non-negative terms, so the total is within (1 + u)^depth - 1 <= depth u / (1 - depth u), u = 2^-53, of the exact sum:
    at most ten ulp of double for three trips.  A dropped or doubled element misses that by many orders of magnitude
    (the smallest of these sums of squares has terms of relative size >> 1e-15)."""
    for active in (None, np.arange(n) % 3 != 2):
        sq = squares(gradient(n), active)
        exact = math.fsum(sq.tolist())
        depth = -(-n // (WG * WG)) + 16
        u = 2.0 ** -53
        assert abs(restate(sq) - exact) <= depth * u / (1.0 - depth * u) * exact, (n, restate(sq), exact)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sgd_clip_norm_is_the_restated_order(n):
    from rag_amd import ops
    dev = torch.device("cuda")
    g = gradient(n)

    def run(active=None):
        p, grad, buf = torch.zeros(n, device=dev), torch.from_numpy(g).to(dev), torch.zeros(n, device=dev)
        if active is None:
            out = ops.sgd_clip_step(p, grad, buf, 1e-2, 0.9, 3e-3, 5.0, True)
        else:
            out = ops.sgd_clip_step_masked(p, grad, buf, torch.from_numpy(active.astype(np.uint8)).to(dev), 1e-2, 0.9, 3e-3, 5.0)
        return int(out.cpu().numpy().view(np.uint32)[0])

    unmasked = run()
    assert unmasked == norm_bits(restate(squares(g))), n
    third = np.arange(n) % 3 != 2                                        # every third element inactive
    assert run(third) == norm_bits(restate(squares(g, third))), n
    assert run(np.ones(n, bool)) == unmasked, n                          # optim.hip: an all-ones mask gives the unmasked sum bit for bit
