"""Training sessions as read_from_file (src/vmisknn/vmis_index.rs:591-686) produces them, from a TSV file or from events already in memory.

TrainingSessions owns an srn_sessions_t handle (include/serenade_hip.h, "training data"):
  from_tsv(path, loader="host")        srn_sessions_from_tsv, or with loader="gpu" srn_sessions_from_tsv_gpu (same sessions, bit for bit)
  from_events(sess, items, times)      srn_sessions_from_events: NumPy arrays, torch tensors on the CPU, or torch tensors on the GPU
                                       (passed by data_ptr(), never copied to the host)
"""
import ctypes as C

import numpy as np

from . import capi


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _event_args(session_ids, item_ids, times, device):
    """-> (keep-alive objects, three pointers, n, flags, stream)."""
    arrs = [session_ids, item_ids, times]
    on_gpu = [_is_torch(a) and a.device.type == "cuda" for a in arrs]
    if any(on_gpu):
        import torch
        if not all(on_gpu):
            raise ValueError("session_ids, item_ids and times must all be GPU tensors or none of them")
        if any(a.device.index != device for a in arrs):
            raise ValueError("the event tensors are not on device %d" % device)
        sess, items, t = (a.contiguous() for a in arrs)
        for a, what in ((sess, "session_ids"), (items, "item_ids")):
            if a.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)):
                raise TypeError("%s must be a 64-bit integer tensor" % what)
        if t.dtype == torch.float64:
            flags = capi.EVENTS_DEVICE
        elif t.dtype == torch.int64:
            flags = capi.EVENTS_DEVICE | capi.EVENTS_TIME_I64
        else:
            raise TypeError("times must be float64 or int64")
        n = sess.numel()
        if items.numel() != n or t.numel() != n:
            raise ValueError("session_ids, item_ids and times differ in length")
        stream = torch.cuda.current_stream(device).cuda_stream
        return (sess, items, t), (sess.data_ptr(), items.data_ptr(), t.data_ptr()), n, flags, stream
    arrs = [a.numpy() if _is_torch(a) else np.asarray(a) for a in arrs]
    sess = np.ascontiguousarray(arrs[0]).astype(np.uint64, copy=False)
    items = np.ascontiguousarray(arrs[1]).astype(np.uint64, copy=False)
    if np.issubdtype(arrs[2].dtype, np.floating):
        t, flags = np.ascontiguousarray(arrs[2], np.float64), 0
    else:
        t, flags = np.ascontiguousarray(arrs[2]).astype(np.int64, copy=False), capi.EVENTS_TIME_I64
    n = len(sess)
    if len(items) != n or len(t) != n:
        raise ValueError("session_ids, item_ids and times differ in length")
    return (sess, items, t), (sess.ctypes.data, items.ctypes.data, t.ctypes.data), n, flags, None


class TrainingSessions:
    """Owns an srn_sessions_t handle: sessions in ascending session id, items ascending, max timestamps."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_tsv(cls, path, loader="host", device=0):
        h = C.c_void_p()
        if loader == "gpu":
            capi.check(capi.lib().srn_sessions_from_tsv_gpu(str(path).encode(), int(device), C.byref(h)))
        elif loader == "host":
            capi.check(capi.lib().srn_sessions_from_tsv(str(path).encode(), C.byref(h)))
        else:
            raise ValueError("loader must be 'host' or 'gpu'")
        return cls(h)

    @classmethod
    def from_events(cls, session_ids, item_ids, times, device=0):
        """Rows in file order; times float (rounded like the file's) or integer seconds (negative -> 0)."""
        keep, (ps, pi, pt), n, flags, stream = _event_args(session_ids, item_ids, times, int(device))
        h = C.c_void_p()
        capi.check(capi.lib().srn_sessions_from_events(C.c_void_p(ps), C.c_void_p(pi), C.c_void_p(pt), n, flags, int(device),
                                                       None if stream is None else C.c_void_p(stream), C.byref(h)))
        del keep
        return cls(h)

    @property
    def handle(self):
        return self._h

    def view(self):
        v = capi.SessionsView()
        capi.check(capi.lib().srn_sessions_view(self._h, C.byref(v)))
        return v

    def arrays(self):
        """-> (sess_off u64[n + 1], items u64[nnz], max_ts u32[n]), copies."""
        v = self.view()
        n = v.n_sessions
        off = np.ctypeslib.as_array(C.cast(v.sess_off, C.POINTER(C.c_uint64)), (n + 1,)).copy()
        nnz = int(off[-1])
        items = np.ctypeslib.as_array(C.cast(v.items, C.POINTER(C.c_uint64)), (nnz,)).copy() if nnz else np.zeros(0, np.uint64)
        ts = np.ctypeslib.as_array(C.cast(v.max_ts, C.POINTER(C.c_uint32)), (n,)).copy() if n else np.zeros(0, np.uint32)
        return off, items, ts

    def length_quantile(self, q=0.995):
        out = C.c_uint64()
        capi.check(capi.lib().srn_sessions_length_quantile(self._h, float(q), C.byref(out)))
        return out.value

    def load_info(self):
        """The GPU loader's counts and stage times (zeros for a host-loaded handle)."""
        out = capi.LoadInfo()
        capi.check(capi.lib().srn_sessions_load_info(self._h, C.byref(out)))
        return {n: getattr(out, n) for n, _ in capi.LoadInfo._fields_}

    def close(self):
        if getattr(self, "_h", None) and capi is not None and getattr(capi, "lib", None) is not None:   # (None at interpreter shutdown)
            capi.lib().srn_sessions_free(self._h)
            self._h = None

    __del__ = close
