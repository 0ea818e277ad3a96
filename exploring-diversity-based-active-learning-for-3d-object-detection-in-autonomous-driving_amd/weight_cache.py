"""The one cache of kernel-format weights ("Packed weights").

A module that folds its BatchNorm and re-lays its weights for a kernel holds one ``PackCache``.  A pack is valid for a
*stamp* -- the device and the identity + version counter of every tensor it was built from -- and is one of several
*variants* under that stamp (one per arithmetic / kernel structure), so flipping ``AL3D_MATH`` back and forth re-packs
nothing, while ``load_state_dict``, an in-place edit or ``.to()`` re-packs everything.  Pure torch; loads no library.
"""
import torch


def versions(*sources):
    """``(data_ptr, _version)`` of every parameter and buffer (``recurse=False``) of the modules among ``sources`` and
    of the bare tensors among them; ``None`` is skipped.  ``load_state_dict`` and in-place edits bump ``_version``, a
    move or a cast changes ``data_ptr``."""
    out = []
    for s in sources:
        if s is None:
            continue
        # a module's own dicts, not parameters() / buffers(): the stamp is taken on every forward
        tensors = (s,) if isinstance(s, torch.Tensor) else (*s._parameters.values(), *s._buffers.values())
        out.extend((t.data_ptr(), t._version) for t in tensors if t is not None)
    return tuple(out)


class PackCache:
    """Packs of one module: ``get`` returns the pack held under ``variant`` for the current stamp, building it on first
    use; a changed stamp drops every held pack.  No other eviction."""

    def __init__(self):
        self._stamp, self._packs = None, {}

    def get(self, device, sources, variant=None, build=None):
        stamp = (torch.device(device), versions(*sources))
        if stamp != self._stamp:
            self._stamp, self._packs = stamp, {}
        if variant not in self._packs:
            self._packs[variant] = build()
        return self._packs[variant]

    def clear(self):
        self._stamp, self._packs = None, {}
