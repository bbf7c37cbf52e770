"""Percentile clipping, max_unorm and LAMB without a GPU: the C-ABI and Python surface exists, the numpy
restatement of the clipped update (tests/optim_norm_helpers.py) reduces to the frozen oracle when clipping
is off, and the combinations the backend refuses raise on the first step."""
import numpy as np
import pytest
import torch

import optim_norm_helpers as nh
from oracle import optim as oref
from oracle import ref


def _bnb():
    import python_src_quants as bnb
    return bnb


def test_percentile_clipping_symbols_and_lamb_classes_exist():
    bnb = _bnb()
    lib = bnb.lib._lib
    for name in ("cpercentile_clipping_g32", "cpercentile_clipping_g16", "cpercentile_clipping_gbf16"):
        assert hasattr(lib, name), name
    for name in ("LAMB", "LAMB8bit", "LAMB32bit"):
        assert issubclass(getattr(bnb.optim, name), bnb.optim.Optimizer2State) and name in bnb.optim.__all__
    assert callable(bnb.functional.percentile_clipping)


def test_lamb_honours_max_unorm_and_keeps_the_reference_defaults():
    bnb = _bnb()
    p = torch.nn.Parameter(torch.zeros(8))
    for cls, bits in ((bnb.optim.LAMB, 32), (bnb.optim.LAMB8bit, 8), (bnb.optim.LAMB32bit, 32)):
        opt = cls([p])
        assert opt.optimizer_name == "lamb"
        assert (opt.args.max_unorm, opt.args.block_wise, opt.args.optim_bits) == (1.0, False, bits)
        assert cls([p], max_unorm=0.25).args.max_unorm == 0.25


def test_percentile_clipping_refuses_other_dtypes():
    F = _bnb().functional
    with pytest.raises(ValueError):
        F.percentile_clipping(torch.zeros(4, dtype=torch.float64), torch.zeros(100), 1)


HP = {"adam": (0.9, 0.999, 1e-8, 1e-3), "momentum": (0.9, 0.0, 0.0, 1e-2), "rmsprop": (0.9, 0.0, 1e-8, 1e-2)}


@pytest.mark.parametrize("kind", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", nh.UNORM_NAMES)
def test_restatement_without_clipping_equals_the_oracle(name, kind):
    rng = np.random.default_rng(11 + nh.UNORM_NAMES.index(name))
    n = 1000
    b1, b2, eps, lr = HP[name]
    p = ref.cast_out((rng.standard_normal(n) * 0.1).astype(np.float32), kind)
    s1 = np.zeros(n, np.float32)
    s2 = np.zeros(n, np.float32) if name == "adam" else None
    for step in range(1, 4):
        g32 = (rng.standard_normal(n) * 0.01).astype(np.float32)
        g32[::50] = 0.0
        g = ref.cast_out(g32, kind)
        skip = step == 2
        ep, e1, e2 = oref.update_32bit(name, g, p, s1, s2, b1, b2, eps, step, lr, 0.01, 1.0, skip, kind)
        # the unorm argument is ignored without max_unorm: any value must give the same bits
        hp, h1, h2, us = nh.update_32bit(name, g, p, s1, s2, b1, b2, eps, step, lr, 0.01, 1.0, skip, kind,
                                         max_unorm=0.0, param_norm=3.0, unorm=123.0)
        assert us == 1.0
        assert np.ascontiguousarray(hp).tobytes() == np.ascontiguousarray(ep).tobytes(), step
        assert h1.tobytes() == e1.tobytes(), step
        if name == "adam":
            assert h2.tobytes() == e2.tobytes(), step
        p, s1, s2 = ep, e1, e2


def test_restatement_update_scale_branches():
    # sqrt(unorm) = 2: above the bound 0.5 * 3 -> scaled; below the bound 1 * 3 -> 1
    assert nh.update_scale("adam", 4.0, 0.5, 3.0, 1e-8) == np.float32(1.5) / np.float32(2.0)
    assert nh.update_scale("adam", 4.0, 1.0, 3.0, 1e-8) == 1.0
    one_state = nh.update_scale("rmsprop", 4.0, 0.5, 3.0, 0.25)
    assert one_state == np.float32(1.75) / np.float32(2.0)                  # + eps on both uses of the bound
    assert nh.update_scale("momentum", 4.0, 0.0, 3.0, 0.0) == 1.0


def _first_step(opt, p):
    p.grad = torch.ones_like(p) * 0.01
    opt.step()


@pytest.mark.parametrize("cls_name", ["Lion", "Adagrad"])
def test_max_unorm_is_refused_for_lion_and_adagrad(cls_name):
    bnb = _bnb()
    p = torch.nn.Parameter(torch.zeros(64))
    opt = getattr(bnb.optim, cls_name)([p], args=nh.optimizer_args(max_unorm=1.0))
    with pytest.raises(NotImplementedError, match="max_unorm"):
        _first_step(opt, p)


def test_max_unorm_is_refused_with_8bit_blockwise_state():
    bnb = _bnb()
    p = torch.nn.Parameter(torch.zeros(4096))
    opt = bnb.optim.Adam8bit([p], args=nh.optimizer_args(optim_bits=8, max_unorm=1.0))
    with pytest.raises(NotImplementedError, match="max_unorm"):
        _first_step(opt, p)
    # LAMB8bit's default block_wise=False ends in the non-blockwise refusal
    q = torch.nn.Parameter(torch.zeros(4096))
    with pytest.raises(NotImplementedError, match="non-blockwise"):
        _first_step(bnb.optim.LAMB8bit([q]), q)


def test_functional_refuses_max_unorm_for_lion_and_adagrad():
    F = _bnb().functional
    t = torch.zeros(8)
    for name in ("lion", "adagrad"):
        with pytest.raises(NotImplementedError, match="max_unorm"):
            F.optimizer_update_32bit(name, t, t, t, 0.9, 1e-8, 1, 1e-3, None, 0.99, unorm_vec=t[:1], max_unorm=1.0)
