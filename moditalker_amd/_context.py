"""The life cycle of a libmtv_hip.so context that the parameter-holder modules share (UNetModel, ViTAutoencoder, CrossAttention,
MotionDecoder, HubertModel): release, pickling / copying without the handle, the weight fingerprint and the upload loop."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


class HipContextMixin:
    """In front of nn.Module in the bases.  The class names its destroy entry point and the attributes that describe the live
    context; it keeps what is its own: building the config struct, the capacity test, its tables call, its training-mode refusals."""

    _destroy = ""                                  # e.g. "mtv_atom_destroy"
    # what describes the live context, and the value each takes in a pickle / copy: the handle is process- and device-local
    _transient = {"_ctx": None, "_key": None, "_fingerprint": None}

    def _release(self):
        if getattr(self, "_ctx", None) is not None:
            getattr(_lib.load(), self._destroy)(self._ctx)       # (binds the context's own device before freeing)
            self._ctx = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # copies / pickles start without a context and create their own lazily (the reference workflow deep-copies the model for
    # its EMA twin, sample.py:226)
    def __getstate__(self):
        st = dict(self.__dict__)
        st.update(self._transient)
        return st

    def _weights_fingerprint(self):
        """(storage, version) of every parameter and buffer.  In-place writes through `.data` (p.data.copy_/lerp_: the usual
        EMA / weight-surgery idiom) do NOT bump `_version`: call `invalidate_weights()` after such writes."""
        return tuple((p.data_ptr(), p._version) for p in list(self.parameters()) + list(self.buffers()))

    def invalidate_weights(self):
        """Force a re-upload of all weights to the HIP context before the next call."""
        self._fingerprint = None

    def _upload_weights(self, ctx, device):
        """Every tensor the context lists (mtv_weight_info), from this module's state_dict, as fp32 on `device`."""
        lib = _lib.load()
        sd = self.state_dict()
        key = C.create_string_buffer(256)
        torch.cuda.synchronize(device)
        with torch.cuda.device(device):
            for i in range(lib.mtv_num_weights(ctx)):
                _lib.check(lib.mtv_weight_info(ctx, i, key, 256, None, None), "mtv_weight_info")
                k = key.value.decode()
                if k not in sd:
                    raise _lib.MtvError(f"library expects weight '{k}' which this module does not hold")
                t = sd[k].detach().to(device=device, dtype=torch.float32).contiguous()
                if t.data_ptr() != sd[k].data_ptr():
                    # a converted / copied temporary is produced on torch's CURRENT stream, while mtv_load_weight copies and
                    # repacks on the NULL stream: finish producing it first (it stays referenced until the call returns,
                    # and the call returns only after its own copy + repack have run)
                    torch.cuda.current_stream(device).synchronize()
                shp = (C.c_int64 * t.dim())(*t.shape)
                _lib.check(lib.mtv_load_weight(ctx, k.encode(), C.c_void_p(t.data_ptr()), t.dim(), shp), f"mtv_load_weight({k})")
        missing = lib.mtv_weights_missing(ctx)
        if missing:
            raise _lib.MtvError(f"{missing} weights missing after upload")
