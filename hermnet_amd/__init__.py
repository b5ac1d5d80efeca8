"""hermnet_amd: MI355X-native engine for HermNet's heterogeneous relational
message-passing hot path."""
from .data import Data, neighbor_search, transform  # noqa: F401
from .hermnet import HVNet, HeteroVertexConv, HTNet, HeteroTriadicConv  # noqa: F401
from .atomic import atom_properties  # noqa: F401
from .stress import energy_forces_stress  # noqa: F401
from .graph import GraphedStep, GraphedMDStep, GraphedBatchMDStep  # noqa: F401
from .md import DeviceMD, DeviceNPT  # noqa: F401
from .relax import DeviceCellRelax, DeviceRelax  # noqa: F401
from .neb import DeviceNEB  # noqa: F401
from .remd import DeviceREMD  # noqa: F401
from .pimd import DevicePIMD  # noqa: F401
from .observe import Frames, MSD, RDF  # noqa: F401
from .metad import Coordination, DeviceMetaD, Distance, bias_on_grid, free_energy  # noqa: F401
from .swapmc import DeviceSwapMD  # noqa: F401
from .nhc import DeviceNHC  # noqa: F401
from .mtk import DeviceMTK  # noqa: F401
from .rmnet import PaiNNModule, PaiNNMessage, PaiNNUpdate, ScaledSiLU, RadialBasis  # noqa: F401

__version__ = "0.1.0"
