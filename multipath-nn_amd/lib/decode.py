"""Decode tables: the 256 floats that 8-bit pixel values stand for (Net.predict / Net.predict_all with ``decode=``; the
lookup itself is mpnn_decode_u8, csrc/decode.hip).  The two named tables are what the reference's prep-data writes into
its datasets: CIFAR pixels are gamma-expanded (scripts/prep-data:93-102), MNIST pixels scaled to [0, 1] (:45-49)."""
import numpy as np

_NAMED = {}


def decode_table(spec):
    """np.float32[256] for a decode spec: 'gamma' (v**2.2 / 255**2.2), 'unit' (v / 255) or an array of 256 values, used
    as it is (converted to float32).  Anything else raises ValueError."""
    if isinstance(spec, str):
        if spec not in ('gamma', 'unit'):
            raise ValueError("decode: %r is no decode table ('gamma', 'unit' or an array of 256 values)" % (spec,))
        if spec not in _NAMED:
            if spec == 'gamma':                      # (the expression of prep-data:94-96: a float64 intermediate)
                t = np.float32(np.arange(256, dtype=np.uint8) ** 2.2 / 255 ** 2.2)
            else:
                t = np.float32(np.arange(256) / 255)
            t.setflags(write=False)
            _NAMED[spec] = t
        return _NAMED[spec]
    if spec is None or isinstance(spec, (bool, int, float)):
        raise ValueError("decode: %r is no decode table ('gamma', 'unit' or an array of 256 values)" % (spec,))
    try:
        t = np.asarray(spec)
        ok = t.shape == (256,) and t.dtype.kind in 'fiu'
    except Exception:
        ok = False
    if not ok:
        raise ValueError("decode: a table is 'gamma', 'unit' or an array of 256 numbers")
    return np.ascontiguousarray(t, dtype=np.float32)


def is_uint8(x):
    """x is a uint8 numpy array or torch tensor."""
    import torch
    return (isinstance(x, torch.Tensor) and x.dtype == torch.uint8) or (isinstance(x, np.ndarray) and x.dtype == np.uint8)


def check_decode_input(what, x, decode):
    """The argument rule of predict / predict_all, checked before an engine is needed: with a decode table the images are
    uint8 (a numpy array or a torch tensor); returns the table (None without decode)."""
    if decode is None:
        return None
    table = decode_table(decode)
    if not is_uint8(x):
        raise ValueError('%s: decode= takes uint8 images (a numpy array or a torch tensor); float images are already '
                         'decoded -- pass them without decode' % what)
    return table
