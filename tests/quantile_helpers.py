"""numpy restatement of cestimate_quantiles_<T> as csrc/quantiles.hip and DESIGN.md §4e define it: blocks of 4096,
IEEE totalOrder inside a block, the fp32 index expression of kernel_quant.cpp:1140-1142, a slot-ordered fp64 sum."""
import numpy as np

F32 = np.float32
BLOCK, SLOTS = 4096, 1024


def order_keys(x32: np.ndarray) -> np.ndarray:
    """The unsigned keys whose order is totalOrder of the fp32 values."""
    u = np.ascontiguousarray(x32, dtype=F32).view(np.uint32)
    return np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000))


def key_values(k: np.ndarray) -> np.ndarray:
    """The inverse of order_keys."""
    return np.where(k >> 31 == 1, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F32)


def total_order_sort(x32: np.ndarray) -> np.ndarray:
    """Ascending along the last axis."""
    return key_values(np.sort(order_keys(x32), axis=-1))


def quantile_indices(valid: int, offset: float) -> np.ndarray:
    """idx[t] = (int)roundf((offset + t * q_interval) * (valid - 1)), every operation rounded to fp32."""
    off = F32(offset)
    q_interval = (F32(1.0) - F32(2.0) * off) / F32(255.0)
    pos = (off + np.arange(256).astype(F32) * q_interval) * F32(valid - 1)
    assert pos.dtype == F32 and np.all(pos >= 0)
    whole = np.trunc(pos)
    return (whole + (pos - whole >= F32(0.5))).astype(np.int64)       # roundf: halves away from zero


def estimate_quantiles(x32: np.ndarray, offset: float) -> np.ndarray:
    """x32: the input converted (exactly) to fp32.  Returns the 256 fp32 entries."""
    x32 = np.ascontiguousarray(x32, dtype=F32).reshape(-1)
    n = x32.size
    blocks = 1 if n < BLOCK else n // BLOCK
    valid = n if n < BLOCK else BLOCK
    idx = quantile_indices(valid, offset)
    picked = total_order_sort(x32[:blocks * valid].reshape(blocks, valid))[:, idx].astype(np.float64)
    slots = np.zeros((min(blocks, SLOTS), 256), np.float64)
    for first in range(0, blocks, SLOTS):          # slot s takes blocks s, s + 1024, ... in that order
        part = picked[first:first + SLOTS]
        slots[:part.shape[0]] += part
    total = np.zeros(256, np.float64)
    for s in range(slots.shape[0]):
        total += slots[s]
    with np.errstate(invalid="ignore"):
        return (total / np.float64(blocks)).astype(F32)


def subsample(code: np.ndarray, num_quantiles: int) -> np.ndarray:
    """functional.estimate_quantiles for num_quantiles < 256: linspace(0, 255, num_quantiles).long()."""
    import torch
    return code[torch.linspace(0, 255, num_quantiles).long().numpy()]


def default_offset(num_quantiles: int) -> float:
    return 1 / 512 if num_quantiles == 256 else 1 / (2 * num_quantiles)
