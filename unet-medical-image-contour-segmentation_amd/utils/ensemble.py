"""Checkpoint ensembles (csrc/ensemble.hip; the reference has no counterpart; DESIGN.md section 3 "Ensembles"): several trained
networks predict the same images and their class probabilities are averaged, each member with an integer weight, before the
argmax.  The probabilities are quantised once (q = rint(p 2^24), the quantiser of test-time augmentation and tiled prediction)
and everything after that is an integer sum, so the result depends on no order of the members.

    Ensemble(models, weights=None)                      the container: members, weights, n_channels, n_classes, eval() / train()
    Ensemble.load(specs, n_channels, n_classes, ...)    members from 'PATH[,arch=A][,w=N]' strings; PATH may be a glob
    parse_member_spec(spec) -> MemberSpec               one such string
    single_model(model)                                 the one network of a bare module or a one-member ensemble, else None

An Ensemble is not an nn.Module and averages nothing itself: BatchPredictor and evaluate take it where they take a network and
run uh_ensemble_add / uh_ensemble_finish (ops.ensemble_add, ops.ensemble_finish).  An ensemble of one member takes the code path
of the bare network: the argmax of the logits and of the quantised probabilities may break ties differently."""
from __future__ import annotations

import dataclasses
import glob as _glob
import os
from typing import Dict, List, Optional, Sequence

import torch

from .distill import ARCHS, teacher_sha256, teacher_shape

MAX_MEMBER_WEIGHT = 255
MAX_TOTAL_WEIGHT = 1024                  # uh_ensemble_finish: total_weight <= 1024 keeps every sum below 2^59


@dataclasses.dataclass(frozen=True)
class MemberSpec:
    """One member of a command line: the checkpoint path (or glob), its architecture (None: the command's --arch) and its weight."""
    path: str
    arch: Optional[str] = None
    weight: int = 1

    def __post_init__(self):
        if not isinstance(self.path, str) or not self.path.strip():
            raise ValueError(f"MemberSpec: the member is the path of a checkpoint file, not {self.path!r}")
        if "," in self.path:
            raise ValueError(f"MemberSpec: the member path may not contain a comma: {self.path!r}")
        if self.arch is not None and self.arch not in ARCHS:
            raise ValueError(f"MemberSpec: arch is one of {', '.join(ARCHS)}, not {self.arch!r}")
        _check_weight(self.weight)
        object.__setattr__(self, "path", self.path.strip())


def _check_weight(w) -> int:
    if isinstance(w, bool) or not isinstance(w, int) or not 1 <= w <= MAX_MEMBER_WEIGHT:
        raise ValueError(f"a member's weight (w=) is an integer in 1..{MAX_MEMBER_WEIGHT}, not {w!r}")
    return w


def parse_member_spec(spec: str) -> MemberSpec:
    """'PATH[,arch=UNet|UNet_S|UNet_T|UNet_SA][,w=N]' -> MemberSpec; the path is the first token and may be a glob, a key that
    is left out keeps its default.  ValueError names what is wrong."""
    if not isinstance(spec, str):
        raise ValueError(f"a member spec is a string 'PATH[,arch=A][,w=N]', not {spec!r}")
    parts = [t.strip() for t in spec.split(",")]
    if not parts[0] or ("=" in parts[0] and parts[0].partition("=")[0] in ("arch", "w")):
        raise ValueError(f"the member path is missing in {spec!r} (it is the first token)")
    kw: Dict = {}
    for tok in parts[1:]:
        key, eq, val = (t.strip() for t in tok.partition("="))
        if key not in ("arch", "w") or not eq or not val:
            raise ValueError(f"{tok!r} is not arch=NAME or w=N in {spec!r} (the path is the first token and may not contain a comma)")
        name = "arch" if key == "arch" else "weight"
        if name in kw:
            raise ValueError(f"{key} is given twice in {spec!r}")
        if key == "w":
            if not val.isdigit():
                raise ValueError(f"the weight (w=) {val!r} in {spec!r} is not an integer in 1..{MAX_MEMBER_WEIGHT}")
            val = int(val)
        kw[name] = val
    return MemberSpec(parts[0], **kw)


def expand_member_specs(specs: Sequence[str]) -> List[MemberSpec]:
    """The specs of a command line, every glob replaced by its matches in sorted order (each with the spec's arch and weight).
    A pattern without a match is a ValueError; a path without glob characters is kept as it is, found or not."""
    out: List[MemberSpec] = []
    for spec in specs:
        m = spec if isinstance(spec, MemberSpec) else parse_member_spec(spec)
        if _glob.has_magic(m.path):
            found = sorted(_glob.glob(m.path))
            if not found:
                raise ValueError(f"the member pattern {m.path!r} matches no file")
            out.extend(dataclasses.replace(m, path=f) for f in found)
        else:
            out.append(m)
    return out


def is_plain_single(specs: Sequence[str]) -> bool:
    """One bare path, no key and no glob: the command line of one model, which runs the one-model code path unchanged."""
    return len(specs) == 1 and isinstance(specs[0], str) and "," not in specs[0] and not _glob.has_magic(specs[0])


class Ensemble:
    """`models`: networks with the same `n_channels` and `n_classes` (architectures and upsampling may differ); `weights`:
    one integer in 1..255 per member (default all 1), at most 1024 in all.  `records`: what Ensemble.load knows of each member's
    file, None for members that were handed over as modules."""

    def __init__(self, models, weights=None, records=None):
        members = list(models)
        if not members:
            raise ValueError("Ensemble needs at least one member")
        for m in members:
            if not isinstance(m, torch.nn.Module) or not hasattr(m, "n_classes") or not hasattr(m, "n_channels"):
                raise ValueError(f"Ensemble: a member is a network with n_channels and n_classes, not {type(m).__name__}")
        if weights is None:
            weights = [1] * len(members)
        weights = list(weights)
        if len(weights) != len(members):
            raise ValueError(f"Ensemble: {len(weights)} weights for {len(members)} members")
        for w in weights:
            _check_weight(w)
        if sum(weights) > MAX_TOTAL_WEIGHT:
            raise ValueError(f"Ensemble: the weights add up to {sum(weights)}, more than {MAX_TOTAL_WEIGHT}")
        first = members[0]
        for k, m in enumerate(members[1:], 1):
            if m.n_classes != first.n_classes:
                raise ValueError(f"Ensemble: member {k} has a head of {m.n_classes} outputs, member 0 one of {first.n_classes}: the "
                                 "members' probabilities are added class by class")
            if m.n_channels != first.n_channels:
                raise ValueError(f"Ensemble: member {k} takes {m.n_channels} input channels, member 0 {first.n_channels}: all members "
                                 "see the same images")
        self.members: List[torch.nn.Module] = members
        self.weights: List[int] = weights
        self.records: Optional[List[Dict]] = list(records) if records is not None else None
        self.n_channels, self.n_classes = int(first.n_channels), int(first.n_classes)

    def __len__(self) -> int:
        return len(self.members)

    @property
    def total_weight(self) -> int:
        return sum(self.weights)

    def eval(self) -> "Ensemble":
        for m in self.members:
            m.eval()
        return self

    def train(self, mode: bool = True) -> "Ensemble":
        for m in self.members:
            m.train(mode)
        return self

    def to(self, *args, **kwargs) -> "Ensemble":
        self.members = [m.to(*args, **kwargs) for m in self.members]
        return self

    @classmethod
    def load(cls, specs: Sequence[str], n_channels: int, n_classes: int, default_arch: str = "UNet", device="cpu") -> "Ensemble":
        """Members from 'PATH[,arch=A][,w=N]' strings (globs expanded).  Bilinear vs transposed-conv upsampling is read off each
        checkpoint's keys (utils.distill.teacher_shape); a head or input-channel mismatch is a ValueError naming the file."""
        from ..checkpoint import load_checkpoint
        from ..train_cli import build_model
        members, weights, records = [], [], []
        for m in expand_member_specs(specs):
            arch = m.arch or default_arch
            shape = teacher_shape(m.path, "member")
            if shape["n_classes"] != int(n_classes) or shape["n_channels"] != int(n_channels):
                raise ValueError(f"the member {m.path!r} has a head of {shape['n_classes']} outputs and takes {shape['n_channels']} input "
                                 f"channels; the ensemble has {int(n_classes)} and {int(n_channels)}")
            model = build_model(arch, int(n_classes), shape["bilinear"])
            try:
                load_checkpoint(model, m.path, device="cpu")
            except RuntimeError as e:
                raise ValueError(f"the member file {m.path!r} does not hold a {arch}{' (bilinear)' if shape['bilinear'] else ''}: "
                                 f"{e}") from None
            model = model.to(memory_format=torch.channels_last).to(device=device)
            model.eval()
            members.append(model)
            weights.append(m.weight)
            records.append({"path": m.path, "arch": arch, "bilinear": shape["bilinear"], "weight": m.weight,
                            "sha256": teacher_sha256(m.path)})
        return cls(members, weights, records)


def single_model(model):
    """The network that runs alone: a bare module, or the member of a one-member ensemble (its weight cancels) -- both take the
    one-model code path.  None for an ensemble that has to be merged."""
    if isinstance(model, Ensemble):
        return model.members[0] if len(model.members) == 1 else None
    return model
