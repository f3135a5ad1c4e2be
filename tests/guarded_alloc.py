"""Device tensors that sit inside a larger allocation, so that a write before or behind them shows.

Belongs here: `guarded` and `untouched`, the arrangement tests/test_gpu_glare.py and tests/fuzz_image.py place d_color, d_out and the
workspace in -- `skip` floats into the allocation (skip = 1 also takes the tensor off its 16-byte alignment: the kernels' one-pixel lane
forms) and GUARD floats before its end.  Importing it loads no library and opens no device: torch is the caller's."""
import numpy as np

GUARD = 64                    # floats behind a tensor that must stay as they were


def guarded(torch, shape, skip, fill):
    """(view, whole): a float32 tensor of `shape` that starts `skip` floats into its allocation and ends GUARD floats before its end,
    all of it filled with `fill`."""
    n = int(np.prod(shape))
    whole = torch.full((skip + n + GUARD,), fill, dtype=torch.float32, device="cuda")
    return whole[skip:skip + n].view(*shape), whole


def untouched(whole, skip, n, fill):
    h = whole.cpu().numpy()
    rest = np.concatenate([h[:skip], h[skip + n:]])
    return len(rest) == skip + GUARD and (np.isnan(rest).all() if np.isnan(fill) else (rest == np.float32(fill)).all())
