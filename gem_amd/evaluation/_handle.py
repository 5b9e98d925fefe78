"""What the evaluation units' handle classes share: the ownership of one library handle, and the ingest of an embedding matrix."""
import ctypes as ct

from gem_amd import _hip


class DeviceHandle(object):
    """Owns one gemhip_*_t: `_h` is the handle a subclass's create call fills, `_destroy` names the library's destroy symbol.
    `with Handle(...) as h:` or close(); close() twice is harmless."""
    _destroy = None

    def __init__(self):
        _hip.require_device()
        self._h = ct.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._h:
            getattr(_hip.lib(), self._destroy)(self._h)
            self._h = ct.c_void_p()


def embedding_matrix(X, d=None):
    """-> (X as contiguous float32 (n, ld), n, d, ld).  d: how many leading columns count (all by default; the rest is padding the device
    never reads)."""
    X = _hip.as_f32(X)
    if X.ndim != 2:
        raise ValueError('X must be (n, d)')
    return X, X.shape[0], X.shape[1] if d is None else int(d), X.shape[1]
