"""GPU: 8-bit optimizer state with one global maximum per state tensor (csrc/optim.hip: k_static8_precondition,
k_static8_finish, k_optimizer_8bit_static), the whole-tensor 8-bit codec (csrc/quant.hip) and the classes on
top (LAMB8bit, <name>8bit(block_wise=False)).

Everything is bit-exact against the numpy restatement in tests/optim_static8_helpers.py, the update norm
included: the restatement adds the fp32 squares in fp64 in the kernels' fixed order, so there is no rounding
slack to allow for.
"""
import numpy as np
import pytest
import torch

import optim_static8_helpers as sh
from helpers import to_numpy, to_torch
from oracle import ref
from oracle.maps import create_dynamic_map

pytestmark = pytest.mark.gpu

KINDS = ["fp32", "fp16", "bf16"]
N_WRAP = sh.SLOTS * sh.CHUNK + 2 * sh.CHUNK + 5    # slots 0..2 take a second chunk, the last one ragged
HP = {"adam": (0.9, 0.999, 1e-8, 1e-3), "momentum": (0.9, 0.0, 0.0, 1e-2), "rmsprop": (0.9, 0.0, 1e-8, 1e-2),
      "lion": (0.9, 0.99, 0.0, 1e-4)}
CASES = {"plain": dict(wd=0.0, gsc=1.0), "wd_gscale": dict(wd=0.01, gsc=0.37),
         "zero_first": dict(wd=0.0, gsc=1.0, zero_first=True)}
CODE1 = np.asarray(create_dynamic_map(signed=True), np.float32)
CODE2 = np.asarray(create_dynamic_map(signed=False), np.float32)


def _F():
    import python_src_quants.functional as F
    return F


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Run:
    """A parameter with global-max 8-bit state on the GPU beside its numpy twin; step() advances both with the
    same gradient, compares every output bit for bit and swaps max / new_max as the optimizer classes do."""

    def __init__(self, dev, name, kind, n, offset=0, wd=0.0, gsc=1.0, zero_first=False, max_unorm=0.0, seed=0,
                 code_idx=None, prefill=0.0):
        self.dev, self.name, self.kind, self.n, self.offset = dev, name, kind, n, offset
        self.wd, self.gsc, self.zero_first, self.max_unorm, self.code_idx = wd, gsc, zero_first, max_unorm, code_idx
        self.two = name == "adam"
        self.rng = np.random.default_rng(seed)
        tot = n + offset                           # offset 1: views that are not 16-byte aligned (scalar paths)
        p = ref.cast_out((self.rng.standard_normal(tot) * 0.1).astype(np.float32), kind)
        self.p, self.tp = p[offset:], to_torch(p, kind, dev)[offset:]
        self.c1, self.tc1 = np.zeros(n, np.uint8), torch.zeros(tot, dtype=torch.uint8, device=dev)[offset:]
        self.c2 = np.zeros(n, np.uint8) if self.two else None
        self.tc2 = torch.zeros(tot, dtype=torch.uint8, device=dev)[offset:] if self.two else None
        self.q1 = torch.from_numpy(CODE1).to(dev)
        self.q2 = torch.from_numpy(CODE2).to(dev) if self.two else None
        self.max1, self.max2 = np.float32(0), (np.float32(0) if self.two else None)
        self.tmax1, self.tnew1 = torch.zeros(1, device=dev), torch.full((1,), prefill, device=dev)
        self.tmax2 = torch.zeros(1, device=dev) if self.two else None
        self.tnew2 = torch.full((1,), prefill, device=dev) if self.two else None
        self.tu = torch.full((1,), prefill, device=dev) if max_unorm > 0 else None
        self.step_no = 0
        self.scales = []

    def grad(self):
        tot = self.n + self.offset
        g32 = (self.rng.standard_normal(tot) * 0.01).astype(np.float32)
        if self.zero_first and self.step_no == 1:
            g32[:] = 0.0
        return ref.cast_out(g32, self.kind)

    def launch(self, tg):
        b1, b2, eps, lr = HP[self.name]
        _F().optimizer_update_8bit(self.name, tg, self.tp, self.tc1, self.tc2, b1, b2, eps, self.step_no, lr, self.q1,
                                   self.q2, self.tmax1, self.tmax2, self.tnew1, self.tnew2, self.wd, self.gsc, self.tu,
                                   self.max_unorm)

    def swap(self):
        self.tmax1, self.tnew1 = self.tnew1, self.tmax1
        self.tmax2, self.tnew2 = self.tnew2, self.tmax2

    def step(self):
        self.step_no += 1
        b1, b2, eps, lr = HP[self.name]
        g = self.grad()
        tg = to_torch(g, self.kind, self.dev)[self.offset:]
        g = g[self.offset:]
        if self.offset:
            assert tg.data_ptr() % 16 == tg.element_size() and self.tc1.data_ptr() % 8 == 1
        param_norm = torch.norm(self.tp.float()).item() if self.max_unorm > 0 else 0.0
        self.launch(tg)
        ep, e1, e2, nm1, nm2, unorm, us = sh.static_step(
            self.name, g, self.p, self.c1, self.c2, CODE1, CODE2, self.max1, self.max2, b1, b2, eps, self.step_no, lr,
            self.wd, self.gsc, self.kind, self.max_unorm, param_norm, self.code_idx)
        tag = (self.name, self.kind, self.n, self.step_no)
        got1 = self.tc1.cpu().numpy()
        got2 = self.tc2.cpu().numpy() if self.two else None
        pick = (lambda a: a) if self.code_idx is None else (lambda a: a[self.code_idx])
        assert np.float32(self.tnew1.item()).tobytes() == np.float32(nm1).tobytes(), (tag, self.tnew1.item(), nm1)
        if self.two:
            assert np.float32(self.tnew2.item()).tobytes() == np.float32(nm2).tobytes(), (tag, self.tnew2.item(), nm2)
        if self.max_unorm > 0:
            print(f"unorm {tag}: gpu {self.tu.item()!r} restatement {float(unorm)!r} update_scale {float(us)!r}")
            assert np.float32(self.tu.item()).tobytes() == np.float32(unorm).tobytes(), tag
        assert np.array_equal(_bits(to_numpy(self.tp, self.kind)), _bits(ep)), tag
        assert np.array_equal(pick(got1), e1), tag
        if self.two:
            assert np.array_equal(pick(got2), e2), tag
        # the next step starts from the stored state (at a sampled size: from the GPU's codes, checked on the sample)
        self.p, self.c1, self.c2, self.max1, self.max2 = ep, got1, got2, nm1, nm2
        self.scales.append(float(us))
        self.swap()
        return g


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sh.NAMES)
def test_three_steps_equal_the_restatement(dev, name, kind, case):
    for n, offset in [(1, 0), (7, 0), (2048, 0), (4096 + 13, 0), (4096 + 13, 1)]:
        run = Run(dev, name, kind, n, offset, seed=n + offset, **CASES[case])
        for _ in range(3):
            run.step()
        if n >= 2048:                              # the states moved off their initial code (after new_max = 0, too)
            assert len(np.unique(run.c1)) > 16


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sh.NAMES)
def test_three_steps_at_the_slot_wrap_size(dev, name, kind):
    """More chunks than slots: slots 0..2 of the precondition take a second chunk, the last one ragged.  p,
    new_max and unorm are compared in full; the codes on the first chunk, the wrapped chunks and the tail, and
    on 32768 random elements (the numpy search over 4 M elements would take seconds per step)."""
    rng = np.random.default_rng(99)
    idx = np.unique(np.concatenate([np.arange(sh.CHUNK), np.arange(sh.SLOTS * sh.CHUNK - 64, N_WRAP),
                                    rng.integers(0, N_WRAP, 32768)]))
    run = Run(dev, name, kind, N_WRAP, seed=5, code_idx=idx, max_unorm=0.05 if name in sh.UNORM_NAMES else 0.0,
              **CASES["wd_gscale"])
    for _ in range(3):
        run.step()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sh.UNORM_NAMES)
@pytest.mark.parametrize("max_unorm", [0.01, 1e3], ids=["clipped", "unclipped"])
def test_max_unorm_equals_the_restatement(dev, name, kind, max_unorm):
    run = Run(dev, name, kind, 4096 + 333, seed=31, max_unorm=max_unorm, wd=0.01, prefill=5.0)
    for _ in range(3):
        run.step()
    # neither case may pass on the other's branch
    assert all(s < 1.0 for s in run.scales) if max_unorm == 0.01 else all(s == 1.0 for s in run.scales), run.scales


def _snapshot(run):
    out = [run.tp, run.tc1, run.tmax1, run.tnew1]
    out += [run.tc2, run.tmax2, run.tnew2] if run.two else []
    out += [run.tu] if run.tu is not None else []
    return [t.clone() for t in out]


@pytest.mark.parametrize("name", ["adam", "momentum"])
def test_a_step_is_deterministic_and_overwrites_its_outputs(dev, name):
    """The same second step from equal inputs: twice on the current stream, once on a side stream (which takes
    its own workspace), and once with new_max and unorm pre-filled with 1e30: equal bits everywhere."""
    n = N_WRAP // 8 + 3

    def second_step(prefill=None, stream=None):
        run = Run(dev, name, "bf16", n, seed=17, max_unorm=0.01, wd=0.01)
        run.step()
        if prefill is not None:
            for t in (run.tnew1, run.tnew2, run.tu):
                if t is not None:
                    t.fill_(prefill)
        run.step_no += 1
        tg = to_torch(run.grad(), "bf16", dev)
        if stream is None:
            run.launch(tg)
        else:
            stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(stream):
                run.launch(tg)
            stream.synchronize()
        return _snapshot(run)

    first = second_step()
    for other in (second_step(), second_step(stream=torch.cuda.Stream(device=dev)), second_step(prefill=1e30)):
        assert len(first) == len(other)
        for a, b in zip(first, other):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("name", sh.NAMES)
def test_every_tail_element_moves(dev, name):
    """n = 7: the reference skips a thread's group of 4 that crosses n; here all 7 entries of p change."""
    F = _F()
    b1, b2, eps, lr = HP[name]
    two = name == "adam"
    p = torch.linspace(0.5, 1.0, 7, device=dev)
    before = p.clone()
    g = torch.full((7,), 0.25, device=dev)
    c = lambda: torch.zeros(7, dtype=torch.uint8, device=dev)   # noqa: E731
    m = lambda: torch.zeros(1, device=dev)                      # noqa: E731
    F.optimizer_update_8bit(name, g, p, c(), c() if two else None, b1, b2, eps, 1, lr, torch.from_numpy(CODE1).to(dev),
                            torch.from_numpy(CODE2).to(dev) if two else None, m(), m() if two else None, m(),
                            m() if two else None)
    assert bool((p != before).all()), (p, before)


def test_large_tensor_equals_its_pieces(dev):
    """More 2048-blocks than workgroups of the update kernel (its grid is every resident workgroup, at most a few
    thousand): each workgroup walks several blocks with the next one's loads in flight.  The per-element
    arithmetic depends on the tensor only through max, new_max and unorm, so with the largest gradient planted
    in every piece the step on the whole tensor equals the steps on its pieces, bit for bit."""
    F = _F()
    pieces, m = 6, 2 ** 22 + 2048 + 13             # 25 M elements, 12 294 blocks
    n = pieces * m
    gen = torch.Generator(device=dev).manual_seed(3)
    p = torch.randn(n, device=dev, generator=gen) * 0.1
    q1, q2 = torch.from_numpy(CODE1).to(dev), torch.from_numpy(CODE2).to(dev)

    def state(k):
        return (torch.zeros(k, dtype=torch.uint8, device=dev), torch.zeros(k, dtype=torch.uint8, device=dev),
                [torch.zeros(1, device=dev) for _ in range(4)])

    whole_p, (w1, w2, wm) = p.clone(), state(n)
    part_p = p.clone()
    parts = [state(m) for _ in range(pieces)]
    for step in (1, 2):
        g = torch.randn(n, device=dev, generator=gen) * 0.01
        g.view(pieces, m)[:, 5] = 1.0              # the maximum of both states, in every piece
        F.optimizer_update_8bit("adam", g, whole_p, w1, w2, 0.9, 0.999, 1e-8, step, 1e-3, q1, q2, wm[0], wm[1], wm[2],
                                wm[3], 0.01, 0.37)
        wm = [wm[2], wm[3], wm[0], wm[1]]
        for i, (c1, c2, pm) in enumerate(parts):
            sl = slice(i * m, (i + 1) * m)
            F.optimizer_update_8bit("adam", g[sl], part_p[sl], c1, c2, 0.9, 0.999, 1e-8, step, 1e-3, q1, q2, pm[0],
                                    pm[1], pm[2], pm[3], 0.01, 0.37)
            pm[:] = [pm[2], pm[3], pm[0], pm[1]]
            assert torch.equal(pm[0], wm[0]) and torch.equal(pm[1], wm[1]), (step, i)
        assert torch.equal(whole_p, part_p), step
        assert torch.equal(w1, torch.cat([c[0] for c in parts])) and torch.equal(w2, torch.cat([c[1] for c in parts]))
    assert len(torch.unique(w1)) > 16 and len(torch.unique(w2)) > 16


# ----------------------------------------------------------------------------- whole-tensor codec
@pytest.mark.parametrize("signed", [True, False], ids=["dynamic", "udynamic"])
@pytest.mark.parametrize("n", [1, 255, 4096 + 13])
def test_codec_equals_the_oracle(dev, signed, n):
    F = _F()
    code = CODE1 if signed else CODE2
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 0.5).astype(np.float32)
    x[::7] = code[rng.integers(0, 256, x[::7].size)]            # exact map entries
    x[::11] = np.float32(1.5) * np.sign(x[::11])                 # outside the map's range
    if not signed:
        x = np.abs(x)
    tcode = torch.from_numpy(code).to(dev)
    q = F.quantize_no_absmax(torch.from_numpy(x).to(dev), tcode)
    assert q.dtype == torch.uint8 and q.shape == (n,)
    assert np.array_equal(q.cpu().numpy(), ref.quantize_8bit_dynamic(code, x).astype(np.uint8))
    codes = rng.integers(0, 256, n).astype(np.uint8)
    d = F.dequantize_no_absmax(torch.from_numpy(codes).to(dev), tcode)
    assert d.dtype == torch.float32 and np.array_equal(_bits(d.cpu().numpy()), _bits(code[codes]))


def test_quantize_dequantize_round_trip(dev):
    F = _F()
    torch.manual_seed(0)
    A = torch.randn(4096 + 13, device=dev) * 3.0
    q, (absmax, code) = F.quantize(A)
    assert q.dtype == torch.uint8 and absmax.item() == A.abs().max().item()
    back = F.dequantize(q, (absmax, code))
    gap = float(np.max(np.diff(CODE1)))
    err = (back - A).abs().max().item()
    print(f"round trip: max error {err!r}, bound {0.5 * gap * absmax.item()!r}")
    assert err <= 0.5 * gap * absmax.item()
    assert torch.equal(F.dequantize(q, absmax=absmax), back)   # the default map


# ----------------------------------------------------------------------------- classes
def test_lamb8bit_with_defaults_takes_a_step(dev):
    import python_src_quants as bnb
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(4096, device=dev) * 0.1)
    before = p.detach().clone()
    opt = bnb.optim.LAMB8bit([p])
    for _ in range(2):
        p.grad = torch.randn_like(p) * 0.01
        opt.step()
    st = opt.state[p]
    assert st["state1"].dtype == torch.uint8 and st["state2"].dtype == torch.uint8
    for key in ("max1", "max2", "new_max1", "new_max2", "unorm_vec"):
        assert st[key].dtype == torch.float32 and st[key].numel() == 1, key
    assert st["max1"].item() > 0 and st["max2"].item() > 0 and st["unorm_vec"].item() > 0
    assert "absmax1" not in st and bool((p.detach() != before).any())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_adam8bit_global_max_equals_hand_rolled_loop(dev, dtype):
    import python_src_quants as bnb
    F = _F()
    n = 4096 + 100
    torch.manual_seed(2)
    p = torch.nn.Parameter((torch.randn(n, device=dev) * 0.1).to(dtype))
    q = p.detach().clone()
    opt = bnb.optim.Adam8bit([p], lr=1e-3, weight_decay=0.01, block_wise=False)
    s1, s2 = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
    q1, q2 = F.create_dynamic_map(signed=True).to(dev), F.create_dynamic_map(signed=False).to(dev)
    m1, m2, n1, n2 = (torch.zeros(1, device=dev) for _ in range(4))
    for step in range(1, 4):
        g = (torch.randn(n, device=dev) * 0.01).to(dtype)
        p.grad = g.clone()
        opt.step()
        F.optimizer_update_8bit("adam", g, q, s1, s2, 0.9, 0.999, 1e-8, step, 1e-3, q1, q2, m1, m2, n1, n2, 0.01)
        m1, n1, m2, n2 = n1, m1, n2, m2
        assert torch.equal(p.detach(), q), step
        st = opt.state[p]
        assert torch.equal(st["state1"], s1) and torch.equal(st["state2"], s2), step
        assert torch.equal(st["max1"], m1) and torch.equal(st["max2"], m2), step


def test_one_state_classes_and_refusals(dev):
    import python_src_quants as bnb
    import optim_norm_helpers as nh
    n = 4096 + 5
    for make in (lambda p: bnb.optim.SGD8bit([p], 0.01, 0.9, block_wise=False),
                 lambda p: bnb.optim.RMSprop8bit([p], block_wise=False),
                 lambda p: bnb.optim.Lion8bit([p], block_wise=False)):
        p = torch.nn.Parameter(torch.randn(n, device=dev) * 0.1)
        before = p.detach().clone()
        opt = make(p)
        for step in range(2):
            p.grad = torch.randn_like(p) * 0.01
            opt.step()
            if step == 0:                          # (Lion's second +-lr undoes its first in half of the elements)
                assert bool((p.detach() != before).all())
        st = opt.state[p]
        assert st["state1"].dtype == torch.uint8 and st["max1"].item() > 0 and "max2" not in st
    refused = [(bnb.optim.RMSprop8bit, dict(args=nh.optimizer_args(optim_bits=8, block_wise=False, max_unorm=1.0))),
               (bnb.optim.Lion8bit, dict(args=nh.optimizer_args(optim_bits=8, block_wise=False, max_unorm=1.0))),
               (bnb.optim.Adagrad8bit, dict(block_wise=False))]
    for cls, kw in refused:
        p = torch.nn.Parameter(torch.zeros(n, device=dev))
        p.grad = torch.ones_like(p)
        with pytest.raises(NotImplementedError):
            cls([p], **kw).step()
    # max_unorm through the classes: momentum with the global max takes it
    p = torch.nn.Parameter(torch.randn(n, device=dev) * 0.1)
    opt = bnb.optim.SGD8bit([p], 0.01, 0.9, args=nh.optimizer_args(optim_bits=8, block_wise=False, max_unorm=0.01))
    p.grad = torch.randn_like(p)
    opt.step()
    assert opt.state[p]["unorm_vec"].sqrt().item() > 0.01 * p.detach().norm().item()


def test_manager_override_of_block_wise_selects_the_global_max_state(dev):
    import python_src_quants as bnb
    mng = bnb.optim.GlobalOptimManager.get_instance()
    mng.initialize()
    try:
        a = torch.nn.Parameter(torch.randn(4096, device=dev) * 0.1)
        b = torch.nn.Parameter(torch.randn(4096, device=dev) * 0.1)
        mng.override_config(b, "block_wise", False)
        mng.register_parameters([a, b])
        opt = bnb.optim.Adam8bit([a, b])
        for p in (a, b):
            p.grad = torch.randn_like(p) * 0.01
        opt.step()
        assert "absmax1" in opt.state[a] and "max1" not in opt.state[a]
        assert "max1" in opt.state[b] and "absmax1" not in opt.state[b] and opt.state[b]["max1"].item() > 0
    finally:
        mng.initialize()


def test_state_dict_roundtrip_continues_bit_identically(dev, tmp_path):
    import python_src_quants as bnb
    torch.manual_seed(1)
    n = 4096 + 100
    p = torch.nn.Parameter((torch.randn(n, device=dev) * 0.1).half())
    opt = bnb.optim.LAMB8bit([p], lr=1e-2)
    for _ in range(2):
        p.grad = torch.randn_like(p) * 0.01
        opt.step()
    path = tmp_path / "opt.pt"
    torch.save(opt.state_dict(), path)
    p2 = torch.nn.Parameter(p.detach().clone())
    opt2 = bnb.optim.LAMB8bit([p2], lr=1e-2)
    opt2.load_state_dict(torch.load(path, weights_only=True))
    for key in ("max1", "max2", "new_max1", "new_max2", "unorm_vec"):
        a, b = opt.state[p][key], opt2.state[p2][key]
        assert b.dtype == torch.float32 and b.numel() == 1 and b.device == p.device and torch.equal(a, b), key
    for key in ("state1", "state2"):
        a, b = opt.state[p][key], opt2.state[p2][key]
        assert b.dtype == torch.uint8 and torch.equal(a, b), key
    assert opt2.state[p2]["step"] == 2
    g = torch.randn_like(p) * 0.01
    p.grad, p2.grad = g.clone(), g.clone()
    opt.step()
    opt2.step()
    assert torch.equal(p.detach(), p2.detach())
    assert torch.equal(opt.state[p]["state1"], opt2.state[p2]["state1"])
    assert torch.equal(opt.state[p]["max2"], opt2.state[p2]["max2"])


def test_lamb8bit_trains_the_two_layer_model(dev):
    """The model, data, steps and criterion of test_optim_norms_gpu.test_lamb_trains_the_two_layer_model."""
    import python_src_quants as bnb
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(784, 256), torch.nn.ReLU(), torch.nn.Linear(256, 10)).to(dev)
    opt = bnb.optim.LAMB8bit(model.parameters(), lr=3e-2)
    x = torch.randn(256, 784, device=dev)
    y = torch.randint(0, 10, (256,), device=dev)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"LAMB8bit losses: first {losses[0]:.4f} last {losses[-1]:.4f}")
    assert losses[-1] < 0.5 * losses[0]
    assert opt.state[model[0].weight]["state1"].dtype == torch.uint8       # 200 704 elements: 8-bit, global max
    assert opt.state[model[0].bias]["state1"].dtype == torch.float32       # below min_8bit_size
