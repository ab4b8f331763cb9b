"""StyleBank: one frozen Y-Net, several adapter sets (styles), one mixed batch.

``YNetTrainer.save_params`` writes a style as the trainable tensors alone (the ``lora_A`` / ``lora_B`` of the adapted encoder
convolutions, a few tens of KB); ``load_separated_params`` puts ONE of them onto the model at a time.  A bank keeps several beside
the model instead: per style and per adapted layer a *shadow* of the layer -- a shallow copy that shares ``weight`` (and ``bias``,
unless the style brings its own) with the model's module, owns its ``lora_A`` / ``lora_B`` and owns its filter cache (``_packed``:
the composed filter in both packed layouts, the Winograd-domain filter with its tag).  The model's own modules, their caches and
their parameter versions are never written: a step graph or an evaluation sweep captured from the model keeps reading exactly what
it read before the bank existed.

``pred_features`` takes a batch SORTED by style and the row bounds of the styles.  The encoder is walked by its own ``forward``
on a shallow copy of its module tree in which every adapted layer is replaced by a dispatcher: that layer runs once per non-empty
style segment, on the segment's contiguous rows, with the kernels ``ynet_conv2d_auto`` picks for that batch size; every other
module of the copy IS the model's module and runs once over all rows.  When one style covers the whole batch the tree holds that
style's shadows themselves (exact ``LoRAConv2d`` objects), so the launches are those of ``predict()`` on a model that loaded the
style.

Served: MoSA / LoRA adapters (``train_net = mosa_r``) and encoder biases, on the plain ('original') and 'embed' networks.
Refused, by name: whole-filter checkpoints (``train_net`` all / train / encoder), decoder tensors (the decoders are shared),
serial / parallel adapter blocks and layers, the semantic adapter, the fusion network, styles of another rank.
"""
import copy
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .ynet import HipConv2d, LoRAConv2d

BASE_STYLE = "base"      # the reserved style name: the model as loaded, with its own lora_A / lora_B; always index 0 of a bank


def sort_by_style(style_index, n_styles):
    """Host bookkeeping of a mixed batch: -> (perm, offsets); ``perm`` is the STABLE order that sorts the agents by style index
    (sorted row j is the caller's row perm[j]); ``offsets`` holds the n_styles + 1 row bounds of the sorted batch (style s owns rows
    offsets[s] .. offsets[s + 1], possibly none).  With one style present perm is the identity."""
    idx = np.asarray(style_index, dtype=np.int64)
    if idx.ndim != 1 or idx.size == 0:
        raise ValueError(f"sort_by_style: expected one style index per agent, got an array of shape {idx.shape}")
    if idx.min() < 0 or idx.max() >= n_styles:
        raise ValueError(f"sort_by_style: style index {int(idx.max() if idx.max() >= n_styles else idx.min())} is outside 0 .. {n_styles - 1}")
    perm = np.argsort(idx, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_styles))])
    return perm, [int(o) for o in offsets]


def _slice_rows(x, lo, hi):
    """Rows lo .. hi of a conv input (a tensor or an ops.LazyCat of tensors)."""
    if isinstance(x, ops.LazyCat):
        return ops.LazyCat([_slice_rows(p, lo, hi) for p in x.parts])
    if not torch.is_tensor(x):
        raise NotImplementedError(f"StyleBank: a {type(x).__name__} input cannot be cut into style segments")
    return x[lo:hi]


class _SegmentedConv(HipConv2d):
    """The dispatcher that stands where an adapted layer stood in the bank's copy of the encoder: rows offsets[s] .. offsets[s + 1]
    of the input go through style s's shadow of the layer.  A HipConv2d by type only (the encoder's walk fuses the ReLU that follows
    into a HipConv2d); it holds no parameter and no filter of its own."""

    def __init__(self, bank, path, base):
        nn.Module.__init__(self)
        self._bank, self._path = [bank], path      # (a list: the bank is no sub-module of this one)
        self.in_channels, self.out_channels, self.kernel_size = base.in_channels, base.out_channels, base.kernel_size

    def extra_repr(self):
        return f"{self._path}: one launch set per style segment"

    def forward(self, x, relu=False, **_):
        bank = self._bank[0]
        offsets = bank._offsets
        if offsets is None or x.shape[0] != offsets[-1]:
            raise RuntimeError(f"StyleBank: layer {self._path} received {x.shape[0]} rows outside pred_features (offsets {offsets})")
        outs = []
        for s in range(len(offsets) - 1):
            lo, hi = offsets[s], offsets[s + 1]
            if hi > lo:
                outs.append(bank._shadows[s][self._path](_slice_rows(x, lo, hi), relu=relu))
        return torch.cat(outs)


def _shadow_tree(module, prefix, replace):
    """A shallow copy of ``module`` in which the sub-modules named in ``replace`` {path: module} are swapped; every branch without a
    replacement is the original object.  The original's ``_modules`` dict is not written."""
    if prefix in replace:
        return replace[prefix]
    if not any(p.startswith(prefix + ".") for p in replace):
        return module
    twin = copy.copy(module)
    twin._modules = OrderedDict((name, _shadow_tree(child, prefix + "." + name, replace)) for name, child in module._modules.items())
    return twin


class StyleBank:
    """``StyleBank(model, styles)``: ``styles`` maps a name to a tuned state dict or to the path of a file written by
    ``YNetTrainer.save_params`` (an iterable of (name, value) pairs is taken too).  ``names[0]`` is BASE_STYLE, the model as loaded;
    the tuned styles follow in the order given.  Everything is validated on the host before a tensor is moved."""

    def __init__(self, model, styles):
        self.model = model
        items = list(styles.items()) if hasattr(styles, "items") else list(styles)
        if not items:
            raise ValueError("StyleBank: the bank is empty (no style besides the base model)")
        names = [BASE_STYLE]
        for name, _ in items:
            if name == BASE_STYLE:
                raise ValueError(f"StyleBank: the name {BASE_STYLE!r} is reserved for the model as loaded and takes no entry")
            if name in names:
                raise ValueError(f"StyleBank: style {name!r} is given twice")
            names.append(name)
        if getattr(model, "network", None) == "fusion":
            raise NotImplementedError("StyleBank: the fusion network (its scene branch runs once for the whole batch) is not served")
        params = dict(model.named_parameters())
        tuned = []
        for name, value in items:
            sd = value if hasattr(value, "keys") else torch.load(value, map_location="cpu", weights_only=False)
            tuned.append(self._validated(name, sd, params))
        self.names = tuple(names)
        paths = sorted({path for sd in tuned for path in sd})
        device = next(model.parameters()).device
        # shadows: [style][path] -> a layer that shares the base filter and owns adapter tensors + filter cache
        self._shadows = []
        for sd in [{}] + tuned:
            layers = OrderedDict()
            for path in paths:
                base = model.get_submodule(path)
                twin = copy.copy(base)
                twin._parameters = OrderedDict(base._parameters)      # weight / bias: the model's own Parameter objects
                for key, t in sd.get(path, {}).items():
                    twin._parameters[key] = nn.Parameter(t.detach().to(device=device, dtype=torch.float32).contiguous().clone(),
                                                         requires_grad=False)
                twin._packed = {}
                layers[path] = twin
            self._shadows.append(layers)
        self._paths = paths
        enc = model.encoder
        self._encoders = [_shadow_tree(enc, "encoder", layers) for layers in self._shadows]
        self._mixed = _shadow_tree(enc, "encoder", {path: _SegmentedConv(self, path, model.get_submodule(path)) for path in paths})
        self._offsets = None
        self.refresh()

    # ---- validation ---------------------------------------------------------------------------------------------------------
    def _validated(self, style, sd, params):
        """{layer path: {parameter name: tensor}} of one style, or the refusal that names the key."""
        model = self.model
        if len(sd) == 0:
            raise ValueError(f"StyleBank: style {style!r} holds no tensor")
        out = {}
        kinds = {}
        for key, t in sd.items():
            if key not in params:
                raise ValueError(f"StyleBank: style {style!r}: {key} is not a parameter of the model")
            if tuple(t.shape) != tuple(params[key].shape):
                raise ValueError(f"StyleBank: style {style!r}: {key} has shape {tuple(t.shape)}, the model's is {tuple(params[key].shape)} "
                                 f"(a style of another rank needs its own model)")
            path, leaf = key.rsplit(".", 1)
            kinds[key] = self._kind(path, leaf, model.get_submodule(path))
        for key, kind in kinds.items():      # a whole-filter checkpoint is named as such before any single key of it
            if kind == "filter":
                raise ValueError(f"StyleBank: style {style!r} replaces whole filters ({key}): it comes from train_net all / train / encoder; "
                                 f"the bank serves adapter-style checkpoints (lora_A / lora_B, encoder biases)")
        for key, kind in kinds.items():
            if kind == "foreign":
                raise ValueError(f"StyleBank: style {style!r}: {key} belongs to no adapted or bias-trainable encoder layer (the decoders and "
                                 f"every other layer are shared by all styles)")
            if kind == "unserved":
                raise NotImplementedError(f"StyleBank: style {style!r}: {key} belongs to a serial / parallel / semantic adapter; the bank "
                                          f"serves MoSA (lora_A / lora_B) adapters and encoder biases")
            path, leaf = key.rsplit(".", 1)
            out.setdefault(path, {})[leaf] = sd[key]
        return out

    @staticmethod
    def _kind(path, leaf, module):
        if any(part in path for part in ("serial_layer", "parallel_layer", "adapters", "semantic_adapter")) or \
                type(module) not in (HipConv2d, LoRAConv2d) and path.startswith("encoder."):
            return "unserved"
        if not path.startswith("encoder.stages."):
            return "foreign"
        if leaf in ("lora_A", "lora_B") and isinstance(module, LoRAConv2d) and module.r > 0:
            return "adapter"
        if leaf == "bias":
            return "adapter"
        return "filter" if leaf == "weight" else "foreign"

    # ---- the style order ------------------------------------------------------------------------------------------------------
    def __len__(self):
        return len(self.names)

    def index(self, name):
        """The index of a style name (an int that is a valid index is handed back)."""
        if isinstance(name, str):
            if name not in self.names:
                raise ValueError(f"StyleBank: unknown style {name!r} (the bank holds {list(self.names)})")
            return self.names.index(name)
        i = int(name)
        if i != name or not 0 <= i < len(self.names):
            raise ValueError(f"StyleBank: unknown style {name!r} (indices 0 .. {len(self.names) - 1})")
        return i

    def indices(self, style):
        """One index per agent from a sequence / array / tensor of names or indices."""
        if torch.is_tensor(style):
            style = style.cpu().tolist()
        return [self.index(s.item() if hasattr(s, "item") else s) for s in list(style)]

    # ---- filters --------------------------------------------------------------------------------------------------------------
    def refresh(self):
        """Compose and pack the filters of every shadow whose tensors changed since its last packing -- at construction all layers of
        a style in ONE ynet_lora_compose_pack_multi call, later only after the base filter's version moved.  Writes the shadows' own
        buffers only; nothing is launched for a bank that is up to date (or before the model is on the device)."""
        device = next(self.model.parameters()).device
        if device.type != "cuda":
            return
        for layers in self._shadows:
            for twin in layers.values():      # (a model moved to the device after the bank was built: the shared tensors went with it)
                for p in twin._parameters.values():
                    if p is not None and p.device != device:
                        p.data = p.data.to(device)
            ops.refresh_filters(nn.ModuleList(layers.values()))
        # ... and of the model's layers that every style shares (the decoders, the embeddings).  The model's ADAPTED layers are left alone:
        # no style reads them (the base style has shadows of its own), and a captured step may be reading their buffers
        ops.refresh_filters(nn.ModuleList(m for name, m in self.model.named_modules()
                                          if name not in self._paths and isinstance(getattr(m, "_packed", None), dict)))

    # ---- the encoder over a style-sorted batch -----------------------------------------------------------------------------------
    def pred_features(self, scene, observed_map, offsets):
        """``model.pred_features`` for a batch sorted by style: ``offsets`` is the host list of len(bank) + 1 row bounds
        (``sort_by_style``).  -> the feature pyramid of all rows."""
        offsets = [int(o) for o in offsets]
        n = observed_map.shape[0]
        if len(offsets) != len(self.names) + 1 or offsets[0] != 0 or offsets[-1] != n or any(b < a for a, b in zip(offsets, offsets[1:])):
            raise ValueError(f"StyleBank.pred_features: offsets {offsets} are not {len(self.names) + 1} ascending row bounds of a batch of {n}")
        present = [s for s in range(len(self.names)) if offsets[s + 1] > offsets[s]]
        x = ops.lazy_cat([scene, observed_map])
        if len(present) == 1:
            return self._encoders[present[0]](x)
        self._offsets = offsets
        try:
            return self._mixed(x)
        finally:
            self._offsets = None
