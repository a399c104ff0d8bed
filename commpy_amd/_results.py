"""The optional results of the calls that take ``want``: an entry point writes one ordered table ``name -> (shape, dtype)``, and its
host and its device function allocate from it -- NumPy arrays or ``DeviceBuf``s of ``prod(shape) * itemsize`` bytes -- pass the
pointer of a wanted result and None for the others, and return the results in table order.  ``want`` is checked by ``_lib.wanted``."""
import math

import numpy as np

from commpy_amd import _lib


def outputs(want, shapes):
    """The zeroed arrays of the results that ``want`` names, in the order of ``shapes`` (name -> (shape, dtype)), and a function that
    gives the pointer of a name's array, None for a result that is not wanted."""
    res = {name: np.zeros(*shapes[name]) for name in shapes if name in want}
    return res, lambda name: _lib.ptr(res[name]) if name in res else None


def device_outputs(want, shapes, given=None):
    """``outputs`` on the device: new ``DeviceBuf``s (not zeroed) as large as the arrays would be.  A buffer of ``given`` (name ->
    ``DeviceBuf`` or None) is used and returned instead of a new one."""
    from commpy_amd.deviceops import DeviceBuf
    given = given or {}
    res = {}
    for name, (shape, dtype) in shapes.items():
        if name in want:
            own = given.get(name)
            res[name] = DeviceBuf(math.prod(shape) * np.dtype(dtype).itemsize) if own is None else own
    return res, lambda name: res[name].ptr if name in res else None


def returned(res, one=False):
    """What a call returns for the results of ``outputs`` / ``device_outputs``: a single result for one name, else a tuple; with
    ``one`` (a 1-D input) the first row of each."""
    out = [v[0] if one else v for v in res.values()]
    return out[0] if len(out) == 1 else tuple(out)
