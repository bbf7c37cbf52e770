"""GPU: percentile clipping, max_unorm and LAMB on the deterministic norms of csrc/optim.hip.

The norms are fixed-order fp64 sums rounded once to fp32.  Their bound against a numpy fp64 sum is 1 fp32
ulp: the squares of the gradient are exact in fp64 (and the update terms are the same fp32 numbers on both
sides), fp64 accumulation of m <= 2^23 non-negative terms errs by at most m * 2^-53 <= 2^-30 relative, far
below half an fp32 ulp, which leaves the final rounding.  Everything downstream of a norm is bit-exact
against the restatement in tests/optim_norm_helpers.py fed with the norm the GPU produced.
"""
import numpy as np
import pytest
import torch

import optim_norm_helpers as nh
from helpers import to_numpy, to_torch
from oracle import ref

pytestmark = pytest.mark.gpu

KINDS = ["fp32", "fp16", "bf16"]
CHUNK, SLOTS = 4096, 1024                          # the partition of csrc/optim.hip
N_WRAP = SLOTS * CHUNK + 2 * CHUNK + 5             # slots 0..2 take a second chunk, the last one ragged
HP = {"adam": (0.9, 0.999, 1e-8, 1e-3), "momentum": (0.9, 0.0, 0.0, 1e-2), "rmsprop": (0.9, 0.0, 1e-8, 1e-2)}


def _F():
    import python_src_quants.functional as F
    return F


_POOL = {}


def _grad(kind, n):
    """The first n of one fixed random gradient per dtype, in `kind` storage (generated once)."""
    if kind not in _POOL:
        rng = np.random.default_rng(KINDS.index(kind))
        _POOL[kind] = ref.cast_out((rng.standard_normal(N_WRAP) * 0.01).astype(np.float32), kind)
    return _POOL[kind][:n]


def _slot(vec, i):
    return vec[i].item()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,offset", [(1, 0), (7, 0), (2048, 0), (4096 + 13, 0), (N_WRAP, 0), (4096 + 13, 1)],
                         ids=["n1", "n7", "n2048", "n4109", "wrap", "unaligned"])
def test_gradient_norm_value_and_determinism(dev, kind, n, offset):
    F = _F()
    g = _grad(kind, n + offset)
    tg = to_torch(g, kind, dev)[offset:]           # offset 1: not 16-byte aligned, the scalar load8 branch
    assert tg.data_ptr() % 16 == (0 if offset == 0 else tg.element_size())
    vec = torch.zeros(100, device=dev)
    F.percentile_clipping(tg, vec, 2)
    got = _slot(vec, 2)
    want = nh.gnorm_sq(g[offset:], kind)
    print(f"gnorm {kind} n={n} offset={offset}: gpu {got!r} numpy {float(want)!r}")
    assert nh.ulps(got, want) <= 1
    vec2 = torch.full((100,), -1.0, device=dev)    # the entry is overwritten, not accumulated into
    F.percentile_clipping(tg, vec2, 2)
    assert np.float32(_slot(vec2, 2)).tobytes() == np.float32(got).tobytes()
    assert torch.equal(vec2[:2], torch.full((2,), -1.0, device=dev)) and bool((vec2[3:] == -1.0).all())


def test_gradient_norm_slots(dev):
    F = _F()
    kind, n = "fp32", 4096 + 13
    tg = to_torch(_grad(kind, n), kind, dev)
    want = nh.gnorm_sq(_grad(kind, n), kind)
    vec = torch.full((100,), 7.0, device=dev)
    gnorm, clip, scale = F.percentile_clipping(tg, vec, 1)          # step 1 seeds every entry
    first = vec.cpu().numpy()
    assert np.all(first == first[0]) and nh.ulps(first[0], want) <= 1
    assert scale == 1.0 and gnorm.item() == clip.item()
    sentinel = torch.arange(1, 101, device=dev, dtype=torch.float32)
    vec = sentinel.clone()
    F.percentile_clipping(tg, vec, 100)
    assert _slot(vec, 0) == first[0] and torch.equal(vec[1:], sentinel[1:])
    F.percentile_clipping(tg, vec, 101)
    assert _slot(vec, 0) == first[0] and _slot(vec, 1) == first[0] and torch.equal(vec[2:], sentinel[2:])


def test_gradient_norm_nan_and_side_stream(dev):
    F = _F()
    kind, n = "bf16", 4096 + 13
    tg = to_torch(_grad(kind, n), kind, dev)
    vec = torch.zeros(100, device=dev)
    F.percentile_clipping(tg, vec, 2)
    side = torch.cuda.Stream(device=dev)
    vec_side = torch.zeros(100, device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                  # another stream takes its own workspace: the same bits
        F.percentile_clipping(tg, vec_side, 2)
    side.synchronize()
    assert torch.equal(vec, vec_side)
    bad = tg.clone()
    bad[n // 2] = float("nan")
    vec = torch.zeros(100, device=dev)
    _, _, scale = F.percentile_clipping(bad, vec, 2)
    assert np.isnan(_slot(vec, 2)) and scale == 1.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", nh.UNORM_NAMES)
@pytest.mark.parametrize("max_unorm", [0.01, 1e3], ids=["clipped", "unclipped"])
def test_update_norm_and_clipped_update_vs_restatement(dev, name, kind, max_unorm):
    F = _F()
    rng = np.random.default_rng(31 + nh.UNORM_NAMES.index(name))
    n = 4096 + 333
    b1, b2, eps, lr = HP[name]
    wd = 0.01
    p = ref.cast_out((rng.standard_normal(n) * 0.1).astype(np.float32), kind)
    s1 = np.zeros(n, np.float32)
    s2 = np.zeros(n, np.float32) if name == "adam" else None
    tp = to_torch(p, kind, dev)
    ts1 = torch.zeros(n, device=dev)
    ts2 = torch.zeros(n, device=dev) if name == "adam" else None
    tu = torch.full((1,), 5.0, device=dev)         # overwritten by every step, never accumulated into
    scales = []
    for step in range(1, 4):
        g32 = (rng.standard_normal(n) * 0.01).astype(np.float32)
        g32[::50] = 0.0
        g = ref.cast_out(g32, kind)
        skip = step == 2
        param_norm = torch.norm(tp.float()).item()
        F.optimizer_update_32bit(name, to_torch(g, kind, dev), tp, ts1, b1, eps, step, lr, ts2, b2, wd, 1.0, tu,
                                 max_unorm=max_unorm, skip_zeros=skip)
        got = tu.item()
        want = nh.unorm_sq(name, g, s1, s2, b1, b2, eps, step, 1.0, kind)
        print(f"unorm {name} {kind} step {step}: gpu {got!r} restatement {float(want)!r}")
        assert nh.ulps(got, want) <= 1, step
        p, s1, s2, us = nh.update_32bit(name, g, p, s1, s2, b1, b2, eps, step, lr, wd, 1.0, skip, kind,
                                        max_unorm=max_unorm, param_norm=param_norm, unorm=got)
        scales.append(float(us))
        assert np.array_equal(to_numpy(tp, kind).view(np.uint8), np.ascontiguousarray(p).view(np.uint8)), step
        assert np.array_equal(ts1.cpu().numpy().view(np.uint32), s1.view(np.uint32)), step
        if name == "adam":
            assert np.array_equal(ts2.cpu().numpy().view(np.uint32), s2.view(np.uint32)), step
    # neither case may pass on the other's branch
    assert all(s < 1.0 for s in scales) if max_unorm == 0.01 else all(s == 1.0 for s in scales), scales


def _clip_grads(n, dev, dtype=torch.float32):
    """8 gradients whose norms fall by 5 % a step, so that none but the 6th (x 100) exceeds the 5th smallest
    recorded norm: percentile clipping scales exactly that one."""
    gen = torch.Generator().manual_seed(5)
    gs = [torch.randn(n, generator=gen) * 0.01 * (1.0 - 0.05 * s) for s in range(1, 9)]
    gs[5] = gs[5] * 100.0
    return [g.to(device=dev, dtype=dtype) for g in gs]


@pytest.mark.parametrize("n", [4096 + 100, 8192])
@pytest.mark.parametrize("bits", [32, 8])
def test_adam_percentile_clipping_equals_hand_rolled_loop(dev, n, bits):
    import python_src_quants as bnb
    F = _F()
    torch.manual_seed(2)
    p = torch.nn.Parameter(torch.randn(n, device=dev) * 0.1)
    q = p.detach().clone()
    opt = (bnb.optim.Adam if bits == 32 else bnb.optim.Adam8bit)([p], lr=1e-3, percentile_clipping=5)
    vec = torch.zeros(100, device=dev)
    if bits == 32:
        s1, s2 = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    else:
        s1, s2 = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
        q1, q2 = F.create_dynamic_map(signed=True).to(dev), F.create_dynamic_map(signed=False).to(dev)
        a1, a2 = (torch.zeros((n + 2047) // 2048, device=dev) for _ in range(2))
    scales = []
    for step, g in enumerate(_clip_grads(n, dev), start=1):
        p.grad = g.clone()
        opt.step()
        scale = F.percentile_clipping(g, vec, step, 5)[2]
        scales.append(float(scale))
        if bits == 32:
            F.optimizer_update_32bit("adam", g, q, s1, 0.9, 1e-8, step, 1e-3, s2, 0.999, 0.0, scale)
        else:
            F.optimizer_update_8bit_blockwise("adam", g, q, s1, s2, 0.9, 0.999, 1e-8, step, 1e-3, q1, q2, a1, a2, 0.0,
                                              gnorm_scale=scale)
        assert torch.equal(p.detach(), q), step
    assert scales[5] < 1.0 and all(s == 1.0 for i, s in enumerate(scales) if i != 5), scales
    st = opt.state[p]
    assert st["state1"].dtype == (torch.float32 if bits == 32 else torch.uint8)
    assert torch.equal(st["gnorm_vec"], vec) and "unorm_vec" not in st


def test_lamb_equals_adam32bit_with_max_unorm_one(dev):
    import python_src_quants as bnb
    torch.manual_seed(4)
    p = torch.nn.Parameter(torch.randn(4096 + 100, device=dev) * 0.1)
    q = torch.nn.Parameter(p.detach().clone())
    lamb = bnb.optim.LAMB([p], lr=1e-2)
    adam = bnb.optim.Adam32bit([q], lr=1e-2, args=nh.optimizer_args(max_unorm=1.0))
    for _ in range(3):
        g = torch.randn_like(p) * 0.01
        p.grad, q.grad = g.clone(), g.clone()
        lamb.step()
        adam.step()
        assert torch.equal(p.detach(), q.detach())
    # the clip was active (an unclipped Adam step differs), so the equality above is not the identity branch
    un, bound = lamb.state[p]["unorm_vec"].sqrt().item(), p.detach().norm().item()
    assert un > bound
    assert torch.equal(lamb.state[p]["unorm_vec"], adam.state[q]["unorm_vec"])


def test_lamb_trains_the_two_layer_model(dev):
    import python_src_quants as bnb
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(784, 256), torch.nn.ReLU(), torch.nn.Linear(256, 10)).to(dev)
    opt = bnb.optim.LAMB(model.parameters(), lr=3e-2)
    x = torch.randn(256, 784, device=dev)
    y = torch.randint(0, 10, (256,), device=dev)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"LAMB losses: first {losses[0]:.4f} last {losses[-1]:.4f}")
    assert losses[-1] < 0.5 * losses[0]
    assert all(opt.state[p]["state1"].dtype == torch.float32 for p in model.parameters())


def test_state_dict_roundtrip_keeps_the_norm_records_fp32(dev, tmp_path):
    import python_src_quants as bnb
    torch.manual_seed(1)
    p = torch.nn.Parameter((torch.randn(4096 + 100, device=dev) * 0.1).half())
    make = lambda: bnb.optim.Adam([p], args=nh.optimizer_args(percentile_clipping=5, max_unorm=1.0))  # noqa: E731
    opt = make()
    for _ in range(2):
        p.grad = (torch.randn_like(p) * 0.01)
        opt.step()
    path = tmp_path / "opt.pt"
    torch.save(opt.state_dict(), path)
    opt2 = make()
    opt2.load_state_dict(torch.load(path, weights_only=True))
    for key, numel in (("gnorm_vec", 100), ("unorm_vec", 1)):
        a, b = opt.state[p][key], opt2.state[p][key]
        assert b.dtype == torch.float32 and b.numel() == numel and b.device == p.device and torch.equal(a, b), key
    assert opt.state[p]["unorm_vec"].item() > 0.0 and opt.state[p]["gnorm_vec"][2].item() > 0.0
