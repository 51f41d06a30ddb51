"""recommendation_amd — MI355X-native (gfx950) hot path for LightGCN-family graph-contrastive
recommenders: CSR SpMM message pass, InfoNCE / prototype contrast, BPR + negative sampler,
as hand-written HIP behind the C ABI of include/gcr.h, with a host-side mirror of the reference's
model-class / loss-function interface (Cmint22/Recommendation: lightgcn.py, ncl.py, ssl4rec.py,
gcl.py, directau.py and univariate/)."""
from . import _lib
from .graph import CsrGraph, SpmmPlan
from . import functional

__all__ = ["CsrGraph", "SpmmPlan", "functional", "_lib", "DiffNetEncoder", "DiffNetModel", "GATConv", "GATRec",
           "GATRecModel", "SAGEConv", "GraphSAGE", "GraphSAGEModel", "GINConv", "GConv", "Encoder", "BootstrapLatent",
           "BootstrapContrast", "BGRLModel"]
__version__ = "0.1.0"


def __getattr__(name):
    """The DiffNet, GAT, GraphSAGE and BGRL classes, imported on first use (their modules pull in the model base, the sampler
    and the optimiser)."""
    if name in ("DiffNetEncoder", "DiffNetModel"):
        from . import diffnet
        return getattr(diffnet, name)
    if name in ("GATConv", "GATRec", "GATRecModel"):
        from . import gat
        return getattr(gat, name)
    if name in ("SAGEConv", "GraphSAGE", "GraphSAGEModel"):
        from . import graphsage
        return getattr(graphsage, name)
    if name in ("GINConv", "GConv", "Encoder", "BootstrapLatent", "BootstrapContrast", "BGRLModel"):
        from . import bgrl
        return getattr(bgrl, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
