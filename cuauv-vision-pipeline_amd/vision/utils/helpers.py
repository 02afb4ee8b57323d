"""Mirror of the reference utils/helpers.py:58-68 (`as_mat`): no UMat exists here, arrays pass through.  And what every image operator
of the mirror is made of: the source check (`image_source`), the host / device fork (`run_operator`), and cv2's exception
(`error`, `as_cv2_error`)."""
import numpy as np

from vision import _vp
from vision.devmat import DeviceMat


class error(Exception):
    """cv2.error of the stand-in (vision.cv2_facade.error is this class)."""


def as_cv2_error(name, call, *args, **kwargs):
    """call(*args, **kwargs); what the mirror refuses (TypeError / ValueError, before anything is launched) is a cv2.error"""
    try:
        return call(*args, **kwargs)
    except (TypeError, ValueError) as e:
        raise error(f"{name}: {e}") from None


def as_mat(mat):
    if isinstance(mat, (np.ndarray, DeviceMat)):
        return mat
    get = getattr(mat, "get", None)
    return get() if callable(get) else mat


def packed_source(src):
    """(image, True) for a DeviceMat, which the operator reads where it is; (packed numpy array, False) for everything else."""
    src = as_mat(src)
    if isinstance(src, DeviceMat):
        return src, True
    return np.ascontiguousarray(src), False


UINT8 = (np.dtype(np.uint8),)


def _said(dtypes, said):
    """the words of image_source's refusals (made when one is raised: a call that passes pays nothing for them)"""
    if said is not None:
        return said
    *first, last = (d.name for d in dtypes)
    words = "expected a non-empty %s (h, w) or (h, w, c) image" % (", ".join(first) + " or " + last if first else last)
    return words, words, "at most 4 channels"


def image_source(mat, dtypes=UINT8, single=None, max_side=None, said=None):
    """The checked source of an image operator and its channel count: a numpy array or a DeviceMat of one of `dtypes` (np.dtype
    objects), (h, w) or (h, w, 1..4), not empty.  single: the words of the refusal of several channels, for an operator that takes
    one ((h, w, 1) comes back as (h, w)).  max_side: the most rows and columns.  said: the facade's words for (the wrong dtype, the
    wrong shape or no pixels, more than 4 channels) where they are not the mirror's; None for the last leaves the channel count to
    the caller."""
    mat = as_mat(mat)
    if not isinstance(mat, (np.ndarray, DeviceMat)) or mat.dtype not in dtypes:
        raise TypeError(_said(dtypes, said)[0])
    shape = mat.shape
    if len(shape) not in (2, 3) or 0 in shape:
        raise TypeError(_said(dtypes, said)[1])
    cn = 1 if len(shape) == 2 else shape[2]
    if cn > 4 and _said(dtypes, said)[2] is not None:
        raise ValueError(_said(dtypes, said)[2])
    if single is not None:
        if len(shape) == 3 and cn == 1:
            mat = mat.reshaped(shape[:2]) if isinstance(mat, DeviceMat) else mat[:, :, 0]
        if mat.ndim != 2:
            raise ValueError(single)
    if max_side is not None and (shape[0] > max_side or shape[1] > max_side):
        raise ValueError(f"the source must be at most {max_side} x {max_side}, as cv2 asserts")
    return mat, cn


def run_operator(src, shape, dtype, host_call, dev_call, binary=False, pair=False):
    """The host / device fork of an image operator, on a checked source.  A DeviceMat gives a DeviceMat that stays in HBM, through
    dev_call(ctx, src_ptr, dst_ptr); a numpy array gives numpy, through host_call(ctx, src_ptr, dst_ptr).  Both return libvp's status.
    pair: two results of the one shape and dtype (the calls take two dst_ptr).  binary: the result is a 0 / 255 mask."""
    ctx = _vp.default_context()
    if isinstance(src, DeviceMat):
        src.refresh_device(ctx)
        out = DeviceMat(ctx, shape, dtype, binary)
        if pair:
            out = out, DeviceMat(ctx, shape, dtype, binary)
            rc = dev_call(ctx, src.dev_ptr, out[0].dev_ptr, out[1].dev_ptr)
        else:
            rc = dev_call(ctx, src.dev_ptr, out.dev_ptr)            # (dev_ptr launches a deferred source)
    else:
        src = np.ascontiguousarray(src)
        out = np.empty(shape, dtype)
        if pair:
            out = out, np.empty(shape, dtype)
            rc = host_call(ctx, src.ctypes.data, out[0].ctypes.data, out[1].ctypes.data)
        else:
            rc = host_call(ctx, src.ctypes.data, out.ctypes.data)
    _vp.check(rc, ctx.handle)
    return out


def device_image(ctx, mat, channels, pending=None):
    """DeviceMat holding `mat` on `ctx`: the image itself when it already lives there, otherwise an upload of the (validated, packed)
    host array (with `pending`, a list: only enqueued - see DeviceMat.from_host).  channels: 1 -> (h, w), 3 -> (h, w, 3), 0 -> either; a trailing axis of length 1 is dropped."""
    if isinstance(mat, DeviceMat):
        if mat.dtype != np.uint8:
            raise TypeError("expected a uint8 image")
        shp = mat.shape
        if len(shp) == 3 and shp[2] == 1 and channels in (0, 1):
            mat = mat.reshaped(shp[:2])
            shp = mat.shape
        if (channels == 3 and not (len(shp) == 3 and shp[2] == 3)) or (channels == 1 and len(shp) != 2) or len(shp) not in (2, 3):
            raise ValueError("expected an (h, w, 3) image" if channels == 3 else "expected an (h, w) image")
        if shp[0] == 0 or shp[1] == 0:
            raise ValueError("empty image")
        mat.refresh_device(ctx)
        return mat
    if not isinstance(mat, np.ndarray) or mat.dtype != np.uint8:
        raise TypeError("expected a uint8 numpy image")
    if mat.ndim == 3 and mat.shape[2] == 1 and channels in (0, 1):
        mat = mat[:, :, 0]
    if (channels == 3 and not (mat.ndim == 3 and mat.shape[2] == 3)) or (channels == 1 and mat.ndim != 2) or mat.ndim not in (2, 3):
        raise ValueError("expected an (h, w, 3) image" if channels == 3 else "expected an (h, w) image")
    if mat.shape[0] == 0 or mat.shape[1] == 0:
        raise ValueError("empty image")
    return DeviceMat.from_host(ctx, mat, pending=pending)


def to_odd(n: int) -> int:
    n = int(n)
    return n if n % 2 == 1 else n + 1
