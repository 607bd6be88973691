"""Guarded, placed operands for the GPU tests that drive a kernel through the POINTERS and batch strides it is handed
(tests/test_gpu_variants.py for the stream kernels, tests/test_gpu_contraction_views.py for the contractions).

Every operand lives in a flat int32 buffer filled with SENTINEL, a quiet NaN with a payload: a read of a word the operand does not
own turns the result into a NaN (also against a zero weight: 0 x NaN = NaN), a write to one changes the sentinel.

  offset_view(values, off)              a contiguous view that starts `off` words past a 16-byte boundary, GUARD words either side
  offset_out(shape, off)                the same for an output: every element the NaN UNWRITTEN until the kernel stores it
  slice_view(values, c0, c_total, off)  values [B, C, H, W] as parent[:, c0:c0 + C] of a [B, c_total, H, W] parent that is itself an
                                        offset_view of sentinels: the channels before and after, the images between (with `pad`
                                        extra words per image) and the guards must keep the sentinel
  slice_out(shape, c0, c_total, off)    the same for an output
  intact(*views)                        every word a view does not own still holds SENTINEL, bit for bit; inputs are unchanged
  written(*outs)                        no element of an output is still UNWRITTEN

and the float64 CPU reference of the three contractions of a bias-free layer (conv_ref64).  Device tensors: needs the GPU."""
import torch
import torch.nn.functional as F

GUARD = 8                       # guard words on either side of a view (8 words = 32 bytes: the view's base keeps its alignment)
SENTINEL = 0x7FC0BEEF           # a quiet NaN with a payload: an over-read shows in the result, an over-write in the guard
UNWRITTEN = 0x7FC0DEAD          # a second payload: an output element the kernel never stored


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _flat(n, off_elems, align):
    start = GUARD + off_elems
    raw = torch.full((start + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    assert raw.data_ptr() % 32 == 0
    return raw, start


def offset_view(values, off_elems, align=16):
    """`values` (float32, any shape) as a contiguous device view that starts off_elems elements past an `align`-byte boundary of a
    flat buffer filled with SENTINEL, GUARD or more sentinel words in front of it and GUARD behind it."""
    values = torch.as_tensor(values, dtype=torch.float32)
    n = values.numel()
    raw, start = _flat(n, off_elems, align)
    view = raw.view(torch.float32)[start:start + n].view(values.shape)
    view.copy_(values)
    assert view.is_contiguous() and view.data_ptr() % align == (4 * off_elems) % align, (view.data_ptr(), off_elems, align)
    view._guard = (raw, start, n)
    return view


def offset_out(shape, off_elems, align=16):
    """an output: every element a NaN (UNWRITTEN) until the kernel writes it"""
    view = offset_view(torch.zeros(tuple(shape)), off_elems, align)
    raw, start, n = view._guard
    raw[start:start + n] = UNWRITTEN
    return view


def guards_intact(*views):
    for k, v in enumerate(views):
        raw, start, n = v._guard
        assert bool((raw[:start] == SENTINEL).all()), "operand %d: the guard words in front of the view were written" % k
        assert bool((raw[start + n:] == SENTINEL).all()), "operand %d: the guard words behind the view were written" % k


def _slice(shape, c0, c_total, off_elems, pad, bs, at):
    B, C = shape[0], shape[1]
    plane = 1
    for s in shape[2:]:
        plane *= s
    assert 0 <= c0 and c0 + C <= c_total and pad >= 0
    row = c_total * plane + pad          # words per image of the parent
    n = B * row
    raw, start = _flat(n, off_elems, 16)
    rows = raw.view(torch.float32)[start:start + n].view(B, row)
    view = rows[:, c0 * plane:(c0 + C) * plane].view(shape)
    owned = torch.zeros(raw.numel(), dtype=torch.bool, device=dev())
    owned[start:start + n].view(B, row)[:, c0 * plane:(c0 + C) * plane] = True
    assert int(owned.sum()) == B * C * plane
    assert (B == 1 or view.stride(0) == row) and tuple(view.shape) == tuple(shape) and view.data_ptr() == raw.data_ptr() + 4 * (start + c0 * plane)
    # the placement the case was written for
    if bs is not None:
        assert view.stride(0) % bs[0] == bs[1], "batch stride %d is not = %d mod %d" % (view.stride(0), bs[1], bs[0])
    if at is not None:
        assert view.data_ptr() % at[0] == at[1], "the view starts %d bytes past a %d-byte boundary, not %d" % (view.data_ptr() % at[0], at[0], at[1])
    return raw, owned, view


def slice_view(values, c0, c_total, off_elems=0, pad=0, bs=None, at=None):
    """`values` [B, C, ...] as parent[:, c0:c0 + C] of a sentinel-filled [B, c_total, ...] parent that starts off_elems words past a
    16-byte boundary, `pad` more sentinel words behind every image of the parent (a batch stride that is no multiple of the plane).
    bs = (m, r): asserts batch stride % m == r (elements); at = (a, r): asserts address % a == r (bytes)."""
    values = torch.as_tensor(values, dtype=torch.float32)
    raw, owned, view = _slice(tuple(values.shape), c0, c_total, off_elems, pad, bs, at)
    view.copy_(values)
    view._placed = (raw, owned, raw.clone())
    return view


def slice_out(shape, c0, c_total, off_elems=0, pad=0, bs=None, at=None):
    """an output slice: every owned element UNWRITTEN until the kernel stores it"""
    raw, owned, view = _slice(tuple(shape), c0, c_total, off_elems, pad, bs, at)
    raw[owned] = UNWRITTEN
    view._placed = (raw, owned, None)
    return view


def intact(*views):
    """Every word outside the views still holds the sentinel; a view made from values (an input) is unchanged altogether."""
    torch.cuda.synchronize()
    for k, v in enumerate(views):
        if hasattr(v, "_guard"):
            guards_intact(v)
            continue
        raw, owned, snapshot = v._placed
        foreign = raw[~owned]
        bad = int((foreign != SENTINEL).sum())
        assert bad == 0, "operand %d: %d words outside the view (neighbouring channels, images between, guards) were written" % (k, bad)
        if snapshot is not None:
            assert torch.equal(raw, snapshot), "operand %d: an input was written" % k


def written(*outs):
    for k, v in enumerate(outs):
        left = int((v.detach().contiguous().view(torch.int32) == UNWRITTEN).sum())
        assert left == 0, "output %d: %d elements were never stored" % (k, left)
        assert not bool(torch.isnan(v).any()), "output %d holds a NaN" % k


def conv_ref64(kind, s, p, x, w, g, groups=1):
    """y, dx and dw of the bias-free layer in float64 on the CPU, from dense copies of the operands (F.conv2d / F.conv_transpose2d,
    torch.autograd.grad)."""
    xr = x.detach().cpu().double().contiguous().requires_grad_(True)
    wr = w.detach().cpu().double().contiguous().requires_grad_(True)
    if kind == "convT":
        yr = F.conv_transpose2d(xr, wr, None, s, p, groups=groups)
    else:
        yr = F.conv2d(xr, wr, None, s, p, groups=groups)
    dx, dw = torch.autograd.grad(yr, (xr, wr), g.detach().cpu().double().contiguous())
    return yr.detach(), dx, dw
