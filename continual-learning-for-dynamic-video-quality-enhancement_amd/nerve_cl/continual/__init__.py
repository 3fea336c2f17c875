"""Continual-learning components around the SR hot path (reference nerve_cl/continual/__init__.py: the same names).
EWC and SynapticIntelligence run their penalty / Fisher arithmetic as flat-bucket HIP kernels; DeviceEpisodicMemory keeps the replay samples in
HBM behind the libnvq replay kernels; ContinualDistillation takes its output and feature terms from the fused kernels of
csrc/distill.hip; AGEM projects the gradient bucket in place with the kernels of csrc/bucket_ops.hip and GEM with those of csrc/gem.hip; the others are host-side loops that only need forward / backward / deepcopy of the model."""
from nerve_cl.continual.memory import EpisodicMemory, StreamingEpisodicMemory
from nerve_cl.continual.device_memory import DeviceEpisodicMemory
from nerve_cl.continual.ewc import EWC, OnlineEWC, SynapticIntelligence
from nerve_cl.continual.maml import MAML, FOMAML, Reptile, ContentAdaptiveMAML
from nerve_cl.continual.distillation import DistillationLoss, ContinualDistillation
from nerve_cl.continual.agem import AGEM
from nerve_cl.continual.gem import GEM

__all__ = ["EpisodicMemory", "StreamingEpisodicMemory", "DeviceEpisodicMemory", "EWC", "OnlineEWC", "SynapticIntelligence", "MAML", "FOMAML",
           "Reptile", "ContentAdaptiveMAML", "DistillationLoss", "ContinualDistillation", "AGEM", "GEM"]
