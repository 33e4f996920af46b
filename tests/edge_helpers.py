"""Helpers shared by the edge modules (test_gpu_sample_edges.py, test_gpu_emulate_edges.py, test_gpu_calibrate_edges.py):
device buffers with sentinel guards on both sides, optionally starting off 16-byte alignment, and bit comparisons.
Importable without a device (torch is imported where a buffer is made)."""
import numpy as np

GUARD = 64                       # elements of sentinel before and after every guarded buffer (a multiple of 16 bytes)
SENTINEL = -777.25


def guarded(eng, rows, shift=0):
    """A (rows, J) view ``shift`` elements into a larger buffer: GUARD + shift sentinels before it, GUARD after."""
    import torch
    flat = torch.full((GUARD + shift + rows * eng.J + GUARD,), SENTINEL, dtype=eng.torch_dtype, device=eng.device)
    view = flat[GUARD + shift:GUARD + shift + rows * eng.J].view(rows, eng.J)
    assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (shift == 0)
    return flat, view


def guards_intact(flat, view):
    head = (view.data_ptr() - flat.data_ptr()) // flat.element_size()
    g = flat.cpu().numpy()
    return bool(np.all(g[:head] == SENTINEL) and np.all(g[head + view.numel():] == SENTINEL))


def put(view, a):
    import torch
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(view.device))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.view(u) == b.view(u)
