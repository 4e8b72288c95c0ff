"""ComposeMaterial — per-object split / apply / concatenate.
Mirrors /root/reference/modules/nclaw/material/preset.py:12-27.  The classical presets of that file (:30-282) live in
classical.py on their own HIP kernels and are re-exported here under the reference's names, so
`from neuma_amd.material.preset import CorotatedElasticity` works as there."""
from typing import Sequence

import torch
import torch.nn as nn
from torch import Tensor

from .classical import (CorotatedElasticity, StVKElasticity, VolumeElasticity, SigmaElasticity, IdentityPlasticity,  # noqa: F401
                        SigmaPlasticity, VonMisesPlasticity, DruckerPragerPlasticity)


class ComposeMaterial(nn.Module):
    def __init__(self, materials, sections: Sequence[int]) -> None:
        super().__init__()
        self.dim = 3
        self.materials = nn.ModuleList(materials)
        self.sections = sections

    def update_sections(self, sections: Sequence[int]) -> None:
        self.sections = sections

    def forward(self, F: Tensor) -> Tensor:
        outs = []
        for m, f in zip(self.materials, torch.split(F, list(self.sections), dim=0)):
            if f.numel() == 0:
                continue
            outs.append(m(f))
        return torch.cat(outs, dim=0)
