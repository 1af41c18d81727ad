"""snac_amd -- MI355X-native batched simulator for ai4ce/SNAC's mobile-construction grid worlds.

The product path is HIP only (libsnac_hip.so behind include/snac_hip.h); nothing here falls back to a CPU
implementation.  See DESIGN.md / INTEGRATION.md.
"""
from ._lib import SnacError, build  # noqa: F401
from . import plans  # noqa: F401

__all__ = ["BatchedDMPEnv", "VectorizedEnvWrapper", "ReplayRing", "RolloutBuffer", "NodePool", "NodePool1D", "NodePool2D", "NodePool3D", "UCTSearch", "SelfPlay", "PriorityTree", "CategoricalSupport", "SoftValue", "PPOLoss", "TDLoss", "SearchLoss", "DeviceMLP", "DeviceAdam", "SnacError", "build", "plans"]


def __getattr__(name):  # torch is imported lazily so that `import snac_amd` stays cheap
    if name == "BatchedDMPEnv":
        from .batched import BatchedDMPEnv

        return BatchedDMPEnv
    if name == "ReplayRing":
        from .replay import ReplayRing

        return ReplayRing
    if name == "RolloutBuffer":
        from .onpolicy import RolloutBuffer

        return RolloutBuffer
    if name in ("NodePool", "NodePool1D", "NodePool2D", "NodePool3D"):
        from . import nodes

        return getattr(nodes, name)
    if name == "UCTSearch":
        from .uct import UCTSearch

        return UCTSearch
    if name == "SelfPlay":
        from .selfplay import SelfPlay

        return SelfPlay
    if name == "PriorityTree":
        from .priority import PriorityTree

        return PriorityTree
    if name == "CategoricalSupport":
        from .distributional import CategoricalSupport

        return CategoricalSupport
    if name == "SoftValue":
        from .sac import SoftValue

        return SoftValue
    if name == "PPOLoss":
        from .ppo import PPOLoss

        return PPOLoss
    if name == "TDLoss":
        from .qloss import TDLoss

        return TDLoss
    if name == "SearchLoss":
        from .search_loss import SearchLoss

        return SearchLoss
    if name == "DeviceMLP":
        from .mlp import DeviceMLP

        return DeviceMLP
    if name == "DeviceAdam":
        from .optim import DeviceAdam

        return DeviceAdam
    if name == "VectorizedEnvWrapper":
        from .vector import VectorizedEnvWrapper

        return VectorizedEnvWrapper
    raise AttributeError(name)
