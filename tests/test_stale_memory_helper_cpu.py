"""The poisoning helper of test_gpu_stale_memory.py, checked on CPU tensors: it writes the pattern
into what `torch.empty` / `torch.empty_like` return, and puts the originals back."""
import struct

import pytest
import torch

import conftest  # noqa: F401  (sys.path)
from stale_memory import PATTERNS, fill_pattern, poisoned_empty, same_bits


def _i32(bits):
    return bits - (1 << 32) if bits >= (1 << 31) else bits


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _f64(bits):
    return struct.unpack("<d", struct.pack("<II", bits, bits))[0]


@pytest.mark.parametrize("bits", [0] + PATTERNS)
def test_wrappers_write_the_pattern_and_are_removed(bits):
    real_empty, real_empty_like = torch.empty, torch.empty_like
    with poisoned_empty(bits) as count:
        assert torch.empty is not real_empty and torch.empty_like is not real_empty_like
        a = torch.empty(3, 5)
        b = torch.empty(7, dtype=torch.float64)
        c = torch.empty(11, dtype=torch.uint8)  # 2 whole words + 3 trailing bytes
        d = torch.empty_like(torch.zeros(4, 2))
        e = torch.empty(0)
        lin = torch.nn.Linear(4, 3)  # torch's own Python-level user of torch.empty: still initialised
        assert count.cpu >= 4 and count.cuda == 0
    assert torch.empty is real_empty and torch.empty_like is real_empty_like
    assert e.numel() == 0
    for t in (a, d):
        assert t.dtype == torch.float32
        assert (t.view(torch.int32) == _i32(bits)).all()
        want = _f32(bits)
        assert torch.isnan(t).all() if want != want else (t == want).all()
    want = _f64(bits)
    assert torch.isnan(b).all() if want != want else (b == want).all()
    assert c[:8].view(torch.int32).tolist() == [_i32(bits)] * 2
    assert c[8:].tolist() == [bits & 0xFF] * 3
    assert torch.isfinite(lin.weight).all() and float(lin.weight.detach().abs().max()) <= 0.5 + 1e-6


def test_pattern_values():
    # what a kernel that reads an unwritten word would see
    assert _f32(0xFFFFFFFF) != _f32(0xFFFFFFFF) and _f32(0x7F800000) == float("inf")
    assert 0.9e38 < _f32(0x7E967699) < 1.1e38
    assert _f64(0xFFFFFFFF) != _f64(0xFFFFFFFF)
    assert 1e306 < _f64(0x7F800000) < 2e306 and 1e301 < _f64(0x7E967699) < 1e302


def test_wrappers_are_removed_after_an_exception():
    real_empty, real_empty_like = torch.empty, torch.empty_like
    with pytest.raises(RuntimeError):
        with poisoned_empty(0x7F800000):
            raise RuntimeError("boom")
    assert torch.empty is real_empty and torch.empty_like is real_empty_like


def test_fill_pattern_skips_what_it_cannot_view():
    t = torch.zeros(6, 4)[:, ::2]
    assert not fill_pattern(t, 0x7F800000) and (t == 0).all()
    assert not fill_pattern(torch.zeros(0), 0x7F800000)


def test_same_bits_reports_rows_and_matches_nan_with_nan():
    a = torch.tensor([[1.0, float("nan")], [2.0, 3.0], [4.0, 5.0]])
    b = a.clone()
    assert same_bits(a, b) == []
    b[2, 1] = float("nan")
    b[0, 0] = 1.5
    assert same_bits(a, b) == [0, 2]
