"""Contiguous views that do not start on a 16-byte boundary: what a caller hands over when it narrows a packed buffer
(`packed_logits[s:e][None]`, `packed_mask[s:e]`, `flat[1:1 + P * N * 4].view(P, N, 4)`).  `is_contiguous()` is true of them, so the
binding accepts them; the kernels that read rows as float4 / float2 / uint4, or store mask bytes as words, must not assume where
they start.  The slack around the view is filled with NaN (integer and bool types: 0xFF bytes), so a kernel that reads a neighbour's
element, or writes past the view, shows it."""
import torch

SLACK = 16      # elements allocated beyond the view's own


def _buffer(t):
    """a 16-byte aligned flat buffer of t.numel() + SLACK elements (+ 16 to align by hand), filled with NaN / 0xFF bytes"""
    buf = torch.empty(t.numel() + SLACK + 16, dtype=t.dtype, device=t.device)
    skip = (-buf.data_ptr() % 16) // t.element_size()
    assert (-buf.data_ptr() % 16) % t.element_size() == 0
    buf = buf[skip:skip + t.numel() + SLACK]
    assert buf.data_ptr() % 16 == 0
    if t.dtype.is_floating_point:
        buf.fill_(float("nan"))
    else:
        buf.view(torch.uint8).fill_(0xFF)
    return buf


def offset_view(t, elems, with_buffer=False):
    """A tensor equal to `t` (same shape, dtype, device; contiguous) whose data_ptr() is `elems * t.element_size()` bytes past a
    16-byte boundary, inside a buffer whose other elements are NaN / 0xFF.  with_buffer: -> (view, buffer) for slack_intact()."""
    assert 0 <= elems <= SLACK and not t.requires_grad
    buf = _buffer(t)
    v = buf[elems:elems + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.shape == t.shape
    assert v.data_ptr() % 16 == (elems * t.element_size()) % 16, (v.data_ptr() % 16, elems, t.element_size())
    assert v.data_ptr() == buf.data_ptr() + elems * t.element_size()
    return (v, buf) if with_buffer else v


def slack_intact(view, buf):
    """the elements of `buf` before and after `view` are still NaN / 0xFF"""
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    assert buf.numel() - view.numel() == SLACK
    if buf.dtype.is_floating_point:
        return bool(torch.isnan(buf[:lo]).all() and torch.isnan(buf[lo + view.numel():]).all())
    b8, e = buf.view(torch.uint8), buf.element_size()      # (bytes: a copy of a bool tensor would turn 0xFF into 1)
    return bool((b8[:lo * e] == 0xFF).all() and (b8[(lo + view.numel()) * e:] == 0xFF).all())
