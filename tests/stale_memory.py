"""Poisoned `torch.empty` / `torch.empty_like` for the stale-memory tests.

The product path takes its outputs, packed images, workspaces, partial-sum blocks and kept
activations from `torch.empty` / `torch.empty_like`, i.e. from whatever the caching allocator
recycles. `poisoned_empty(bits)` replaces both (as attributes of the `torch` module, which is how
every nfs_amd module reaches them) by wrappers that fill each new tensor with a 32-bit pattern, so
a kernel that reads a word it never wrote sees NaN / Inf / a huge value instead of the small
finite leftovers of a fresh test process.
"""
import contextlib

import torch

# 0 = the baseline; all-ones NaN, +Inf and 1e38 in fp32 (NaN / 1.4e306 / 6e301 read as float64):
# the non-zero ones are test_gpu_lds_poison.py's
PATTERNS = [0xFFFFFFFF, 0x7F800000, 0x7E967699]


def fill_pattern(t, bits):
    """Write the 32-bit pattern over the bytes of a contiguous tensor through an int32 view (a
    trailing numel % 4 bytes of a uint8 buffer get the low byte). Returns False for a tensor it
    leaves alone (empty, non-contiguous)."""
    if t.numel() == 0 or not t.is_contiguous():
        return False
    raw = t.detach().view(-1).view(torch.uint8)
    n4 = raw.numel() // 4
    signed = bits - (1 << 32) if bits >= (1 << 31) else bits
    if n4:
        raw[:4 * n4].view(torch.int32).fill_(signed)
    if raw.numel() > 4 * n4:
        raw[4 * n4:].fill_(bits & 0xFF)
    return True


class Poison:
    """What one `poisoned_empty` block filled: `cuda` / `cpu` = number of tensors."""

    def __init__(self):
        self.cuda = 0
        self.cpu = 0


@contextlib.contextmanager
def poisoned_empty(bits):
    real_empty, real_empty_like = torch.empty, torch.empty_like
    count = Poison()

    def note(t):
        if isinstance(t, torch.Tensor) and t.layout == torch.strided and fill_pattern(t, bits):
            if t.device.type == "cuda":
                count.cuda += 1
            else:
                count.cpu += 1
        return t

    def empty(*args, **kwargs):
        return note(real_empty(*args, **kwargs))

    def empty_like(*args, **kwargs):
        return note(real_empty_like(*args, **kwargs))

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield count
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like


def same_bits(a, b):
    """Rows (first dimension) where a and b differ other than NaN against NaN."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.numel() == 0:
        return []
    bad = (a != b) & ~(torch.isnan(a) & torch.isnan(b)) if a.is_floating_point() else (a != b)
    if a.dim() == 0:
        return [0] if bool(bad) else []
    return bad.reshape(a.shape[0], -1).any(dim=1).nonzero().flatten().tolist()
