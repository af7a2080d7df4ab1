"""serenade_amd -- MI355X (gfx950) implementation of Serenade's VMIS-kNN `predict_next` hot path.

The package holds only what that path needs: the HIP kernels + C ABI (csrc/, built into
libserenade_hip.so), a ctypes binding (capi), the host-side mirror of the reference interface
(vmisknn), training data from TSV files or in-memory events on the GPU (ingest), the offline evaluation loop and hyper-parameter search on the GPU (evaluation, hpo), a click log's split by time and the walk-forward backtest on the GPU (prepare) and the synthetic workload generator
used by bench.py (synth)."""
from .vmisknn import CSR, ItemScore, VMISIndex, SerenadeError, predict, predict_batch, predict_batch_debug, predict_batch_device, predict_batch_device_excl, reserve  # noqa: F401
from .evaluation import EvalSet, evaluate  # noqa: F401
from .ingest import TrainingSessions  # noqa: F401
from .serving import SessionHarvest, TrafficSplit, arms_model, harvest_model, recommend_batch_split, refreshed_index, replay, split_compare  # noqa: F401

_PREPARE = ("Split", "backtest", "read_events", "split_events", "split_model")


def __getattr__(name):   # prepare is also a command (python -m serenade_amd.prepare): imported at first use, so that runpy finds it unloaded
    if name == "prepare" or name in _PREPARE:
        import importlib
        mod = importlib.import_module(".prepare", __name__)
        return mod if name == "prepare" else getattr(mod, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


__all__ = ["CSR", "ItemScore", "VMISIndex", "SerenadeError", "predict", "predict_batch", "predict_batch_debug", "predict_batch_device", "predict_batch_device_excl", "reserve",
           "EvalSet", "evaluate", "TrainingSessions", "SessionHarvest", "harvest_model", "refreshed_index", "replay",
           "TrafficSplit", "recommend_batch_split", "arms_model", "split_compare", *_PREPARE]
