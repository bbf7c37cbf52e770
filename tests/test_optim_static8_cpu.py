"""8-bit optimizer state with one global maximum per state tensor, without a GPU: the numpy restatement of a
step (tests/optim_static8_helpers.py) is pinned to the frozen oracle, the Python and C surface exists, and the
combinations the backend refuses raise."""
import math
import os
import re

import numpy as np
import pytest
import torch

import optim_static8_helpers as sh
from oracle import optim as oref
from oracle import ref
from oracle.maps import create_dynamic_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = {"adam": (0.9, 0.999, 1e-8, 1e-3), "momentum": (0.9, 0.0, 0.0, 1e-2), "lion": (0.9, 0.99, 0.0, 1e-4),
      "rmsprop": (0.9, 0.0, 1e-8, 1e-2)}
PIN = ([(name, kind) for name in ("adam", "momentum") for kind in ("fp32", "fp16", "bf16")] + [("lion", "fp32")])


def _maps():
    return (np.asarray(create_dynamic_map(signed=True), np.float32),
            np.asarray(create_dynamic_map(signed=False), np.float32))


@pytest.mark.parametrize("wd,gsc", [(0.0, 1.0), (0.01, 0.37)], ids=["plain", "wd_gscale"])
@pytest.mark.parametrize("n", [2048, 1000])
@pytest.mark.parametrize("name,kind", PIN, ids=[f"{a}-{b}" for a, b in PIN])
def test_restatement_equals_the_blockwise_oracle_on_one_block(name, kind, n, wd, gsc):
    """With a single 2048-block the block's absmax is the global maximum, so the two state kinds coincide: p,
    the codes and new_max == absmax[0], bit for bit, over 3 steps (finite gradients, max_unorm = 0).  RMSprop
    is left out: its p update associates differently in the reference's two kernels, as does Lion's outside
    fp32 (the blockwise kernel rounds lr * sign to the storage type)."""
    rng = np.random.default_rng(7 + sh.NAMES.index(name))
    code1, code2 = _maps()
    b1, b2, eps, lr = HP[name]
    two = name == "adam"
    p = ref.cast_out((rng.standard_normal(n) * 0.1).astype(np.float32), kind)
    c1 = np.zeros(n, np.uint8)
    c2 = np.zeros(n, np.uint8) if two else None
    a1 = np.zeros(1, np.float32)
    a2 = np.zeros(1, np.float32) if two else None
    for step in range(1, 4):
        g = ref.cast_out((rng.standard_normal(n) * 0.01).astype(np.float32), kind)
        ep, e1, e2, ea1, ea2 = oref.update_8bit_blockwise(name, g, p, c1, c2, code1, code2, a1, a2, b1, b2, eps, step,
                                                          lr, wd, gsc, False, kind)
        hp, h1, h2, nm1, nm2, unorm, us = sh.static_step(name, g, p, c1, c2, code1, code2, a1[0], a2[0] if two else None,
                                                         b1, b2, eps, step, lr, wd, gsc, kind)
        assert unorm is None and us == 1.0
        assert np.ascontiguousarray(hp).tobytes() == np.ascontiguousarray(ep).tobytes(), step
        assert h1.tobytes() == e1.tobytes(), step
        assert np.float32(nm1).tobytes() == ea1[0].tobytes(), step
        if two:
            assert h2.tobytes() == e2.tobytes(), step
            assert np.float32(nm2).tobytes() == ea2[0].tobytes(), step
        p, c1, c2, a1, a2 = ep, e1, e2, ea1, ea2
    assert len(np.unique(c1)) > 16                 # the states moved off their initial code


def test_fixed_order_sum_is_the_sum():
    rng = np.random.default_rng(3)
    for n in (1, 7, 4096 + 13, sh.SLOTS * sh.CHUNK + 2 * sh.CHUNK + 5):
        t = rng.random(n)
        got, want = sh.fixed_order_sum(t), math.fsum(t.tolist())
        assert abs(got - want) <= 1e-12 * want, n


def test_restatement_update_scale_branches():
    # sqrt(unorm) = 2: above the bound 0.5 * 3 -> scaled; below the bound 1 * 3 -> 1; no eps on the bound
    assert sh.update_scale(4.0, 0.5, 3.0) == np.float32(1.5) / np.float32(2.0)
    assert sh.update_scale(4.0, 1.0, 3.0) == 1.0
    assert sh.update_scale(None, 0.0, 3.0) == 1.0


def test_functional_surface_and_refusals():
    import python_src_quants.functional as F
    for fn in ("optimizer_update_8bit", "quantize", "dequantize", "quantize_no_absmax", "dequantize_no_absmax"):
        assert callable(getattr(F, fn)), fn
    t, c = torch.zeros(8), torch.zeros(8, dtype=torch.uint8)
    m, q = torch.zeros(1), torch.zeros(256)
    for name in ("rmsprop", "lion"):
        with pytest.raises(NotImplementedError, match="max_unorm"):
            F.optimizer_update_8bit(name, t, t, c, None, 0.9, 0.99, 1e-8, 1, 1e-3, q, None, m, None, m.clone(), None,
                                    unorm_vec=m.clone(), max_unorm=1.0)
    with pytest.raises(ValueError, match="unorm_vec"):
        F.optimizer_update_8bit("adam", t, t, c, c.clone(), 0.9, 0.99, 1e-8, 1, 1e-3, q, q, m, m.clone(), m.clone(),
                                m.clone(), max_unorm=1.0)
    with pytest.raises(ValueError):                # no global-max kernel for adagrad, as in the reference
        F.optimizer_update_8bit("adagrad", t, t, c, None, 0.0, 0.0, 1e-8, 1, 1e-3, q, None, m, None, m.clone(), None)
    with pytest.raises(TypeError):                 # no CPU implementation of this path
        F.optimizer_update_8bit("momentum", t, t, c, None, 0.9, 0.0, 0.0, 1, 1e-3, q, None, m, None, m.clone(), None)


def test_classes_refuse_the_path_for_a_parameter_off_the_gpu():
    import python_src_quants as bnb
    # a parameter that is not on a GPU: the refusal of non-blockwise state stays
    for make in (lambda p: bnb.optim.Adam8bit([p], block_wise=False),
                 lambda p: bnb.optim.SGD8bit([p], 0.1, 0.9, block_wise=False)):
        p = torch.nn.Parameter(torch.zeros(4096))
        opt = make(p)
        p.grad = torch.ones_like(p) * 0.01
        with pytest.raises(NotImplementedError, match="non-blockwise"):
            opt.step()


def test_header_declares_the_static_and_codec_symbols():
    txt = open(os.path.join(ROOT, "include", "bnb_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", txt))
    want = {f"c{name}_static_8bit_grad_{bits}" for name in sh.NAMES for bits in ("32", "16", "bf16")}
    assert len(want) == 12 and want <= declared, sorted(want - declared)
    assert {"cquantize", "cdequantize"} <= declared
    import python_src_quants as bnb
    for sym in sorted(want | {"cquantize", "cdequantize"}):
        assert hasattr(bnb.lib._lib, sym), sym
