"""LAMB, ref:python_src_quants/optim/lamb.py (kernel "lamb": the Adam entry points with the update's L2 norm
clipped against max_unorm * ||p||), with fp32 states or, in LAMB8bit, 8-bit states.

The reference's three classes accept ``max_unorm`` and then pass the literal 1.0 to the base class
(ref:optim/lamb.py:71, 135, 199), so the argument has no effect there; here it is honoured (the default,
1.0, gives the reference's behaviour).  ``bias_correction`` and ``adam_w_mode`` are accepted and unused, as
in the reference.  LAMB8bit keeps the reference's ``block_wise=False`` default: parameters of at least
``min_8bit_size`` elements keep 8-bit states quantised against one global maximum per state tensor
(F.optimizer_update_8bit), the one 8-bit state kind that takes ``max_unorm``.  That path runs on a GPU only; a
parameter that is not on one is refused.
"""
from .optimizer import Optimizer2State


class LAMB(Optimizer2State):
    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 amsgrad=False, adam_w_mode=True, optim_bits=32, args=None, min_8bit_size=4096,
                 percentile_clipping=100, block_wise=False, max_unorm=1.0):
        if amsgrad:
            raise NotImplementedError("amsgrad is not supported")
        super().__init__("lamb", params, lr, betas, eps, weight_decay, optim_bits, args, min_8bit_size,
                         percentile_clipping, block_wise, max_unorm=max_unorm)


class LAMB8bit(Optimizer2State):
    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 amsgrad=False, adam_w_mode=True, args=None, min_8bit_size=4096, percentile_clipping=100,
                 block_wise=False, max_unorm=1.0):
        if amsgrad:
            raise NotImplementedError("amsgrad is not supported")
        super().__init__("lamb", params, lr, betas, eps, weight_decay, 8, args, min_8bit_size,
                         percentile_clipping, block_wise, max_unorm=max_unorm)


class LAMB32bit(Optimizer2State):
    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 amsgrad=False, adam_w_mode=True, args=None, min_8bit_size=4096, percentile_clipping=100,
                 block_wise=False, max_unorm=1.0):
        if amsgrad:
            raise NotImplementedError("amsgrad is not supported")
        super().__init__("lamb", params, lr, betas, eps, weight_decay, 32, args, min_8bit_size,
                         percentile_clipping, block_wise, max_unorm=max_unorm)
