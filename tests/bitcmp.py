"""Bit comparison of float32 results: the views and predicates the tests compare device output with the oracle through.

Belongs here: a way to look at float32 values as bits, or to call two such arrays equal.  Two kinds, never to be mixed up: exact
on bits (`ibits`, `bits`), and exact on bits except that any two NaNs are equal (`nan_eq`, `canon`, `same`), for values whose NaN
payloads x86 and gfx950 choose differently.  Every function takes numpy arrays and (host or device) torch tensors alike."""
import numpy as np

f32 = np.float32
QUIET_NAN = 0x7FC00000


def host(a):
    """A tensor's values as a numpy array; anything else through np.asarray."""
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def ibits(a):
    """The float32 bits of an array or tensor as an int32 numpy array (a uint32 view compares the same)."""
    return np.ascontiguousarray(host(a), f32).view(np.int32)


def bits(a):
    """ibits of a float32 result; a result of any other type (triangle indices, RGB8, counts) as it is."""
    a = host(a)
    return ibits(a) if a.dtype == f32 else np.ascontiguousarray(a)


def nan_eq(a, b):
    """Elementwise bit equality where any two NaNs count as equal (x86 and gfx950 NaN payloads differ)."""
    a, b = np.asarray(host(a), f32), np.asarray(host(b), f32)
    return (ibits(a) == ibits(b)) | (np.isnan(a) & np.isnan(b))


def canon(a):
    """ibits with every NaN mapped to one pattern (IEEE leaves NaN payloads to the implementation)."""
    b = ibits(a).copy()
    b[np.isnan(np.asarray(host(a), f32))] = QUIET_NAN
    return b


def same(a, b):
    """Two arrays of one shape whose float32 values are equal on bits, NaN = NaN."""
    return a.shape == b.shape and bool(np.array_equal(canon(a), canon(b)))


def same_exact(a, b):
    """Two results of one call, exact on bits and compared where they are: tensors (float32 as raw bits), or tuples of tensors / None."""
    import torch
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_exact(x, y) for x, y in zip(a, b))
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)
