"""What every batch wrapper of this package does before and after its one
native call: turn tensors, addresses and Python lists into the arguments
include/uplink_ec.h takes, make the caller's stream current for the tensors it
allocates, and wait where a result is read back.

Streams.  `stream` is None (torch's current stream), a torch stream, or a raw
hipStream_t handle.  A raw handle is a stream torch knows nothing of: its
allocations and copies do not follow it, so wherever a wrapper reads a result
back or frees a buffer the queued kernels still read, it has to wait for the
device first.  That rule lives in wait_if_raw and nowhere else.

torch is imported inside the functions: the host tests import the package
without a device.
"""
from __future__ import annotations

import contextlib
import ctypes


def addr(x):
    """the device address of a tensor, or the address itself"""
    return x.data_ptr() if hasattr(x, "data_ptr") else int(x)


def stream_handle(stream):
    """the hipStream_t a native call takes"""
    if stream is None:
        try:
            import torch
            return torch.cuda.current_stream().cuda_stream
        except Exception:
            return None
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream


def ctx_of(scheme_or_ctx):
    return scheme_or_ctx.ctx if hasattr(scheme_or_ctx, "ctx") else scheme_or_ctx


# ---- argument arrays.  Each has max(n, 1) entries: an empty list is still a valid pointer.
def ptr_array(values, n=None, noun="buffer", per="segment"):
    """void*[n] of tensors, addresses or None (a null pointer)"""
    values = [0 if x is None else x.data_ptr() if hasattr(x, "data_ptr") else int(x) for x in values]
    if n is not None and len(values) != n:
        raise ValueError(f"one {noun} per {per}")
    return (ctypes.c_void_p * max(len(values), 1))(*values)


def size_array(values, n=None, noun="size", per="segment", one_error=False):
    """size_t[n]: ValueError "one <noun> per <per>" for another length and
    "a <noun> is negative" for a negative value -- or, with one_error, "one
    non-negative <noun> per <per>" for both"""
    values = [int(x) for x in values]
    wrong_length = n is not None and len(values) != n
    negative = bool(values) and min(values) < 0
    if one_error and (wrong_length or negative):
        raise ValueError(f"one non-negative {noun} per {per}")
    if wrong_length:
        raise ValueError(f"one {noun} per {per}")
    if negative:
        raise ValueError(f"a {noun} is negative")
    return (ctypes.c_size_t * max(len(values), 1))(*values)


def int_array(values, n=None, noun="number", per="segment"):
    """int[n] (piece numbers and counts: the library checks their range)"""
    values = [int(x) for x in values]
    if n is not None and len(values) != n:
        raise ValueError(f"one {noun} per {per}")
    return (ctypes.c_int * max(len(values), 1))(*values)


# ---- streams
def stream_scope(stream):
    """context manager: a torch stream made current, so that the tensors
    allocated inside belong to it; nothing for None and for a raw handle"""
    if hasattr(stream, "cuda_stream"):
        import torch
        return torch.cuda.stream(stream)
    return contextlib.nullcontext()


def wait_if_raw(stream):
    """A raw stream handle is not a stream torch's copies and frees follow:
    wait for the device before reading back what was queued on it, or letting
    go of what it still reads."""
    if stream is not None and not hasattr(stream, "cuda_stream"):
        import torch
        torch.cuda.synchronize()


def read_back(tensor, stream):
    """the values of a device tensor filled on `stream` (a copy on the current
    stream: it waits for a torch stream by itself)"""
    wait_if_raw(stream)
    return tensor.cpu().tolist()


def default_device():
    import torch
    return torch.device("cuda", torch.cuda.current_device())
