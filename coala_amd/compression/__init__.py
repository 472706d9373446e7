"""MI355X-native model-update compression for COALA (the package the reference leaves empty:
/root/reference/coala/compression/__init__.py is 0 bytes).

Public surface:
  CompressionClientMixin / CompressionServerMixin — hook mixins (plugin.py)
  UpdateCodec, CompressedUpdate                    — state_dict codec + picklable carrier (codec.py)
  CompressedModel, compress_model                  — download direction: compressed global model (download.py)
  CodecPlan, Encoded                               — batched device-level API over the C ABI (plan.py)
  k_for, SegmentTable                              — CodecSpec v1 host logic (spec.py)

The names are imported from their modules on first use: a process that only checks blobs
(`import coala_amd.compression.validate`) does not load torch.
"""
from importlib import import_module

from . import wire

_HOMES = {"codec": ("CompressedUpdate", "FlatState", "HipBackend", "UpdateCodec", "flatten_state", "module_with_state"),
          "download": ("CompressedModel", "compress_model", "skeleton_of"),
          "pipeline": ("SplitPipeline", "split_lanes"),
          "plan": ("CodecPlan", "Encoded"),
          "plugin": ("CompressionClientMixin", "CompressionServerMixin"),
          "spec": ("ALIGN", "RAW_BITS", "SegmentTable", "SubTable", "k_for")}
_HOME_OF = {name: home for home, names in _HOMES.items() for name in names}

__all__ = ["wire", *_HOME_OF]


def __getattr__(name):
    if name not in _HOME_OF:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    value = globals()[name] = getattr(import_module("." + _HOME_OF[name], __name__), name)
    return value
