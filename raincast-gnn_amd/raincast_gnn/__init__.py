"""raincast_gnn -- MI355X-native (gfx950) GINEConv message-passing engine for the
station-graph precipitation GNN of SohirMaskey/raincast-gnn.

The drop-in is :class:`raincast_gnn.nn.GINEConv` (replaces ``torch_geometric.nn.GINEConv``
at models/gnn.py:5); :mod:`raincast_gnn.models` rebuilds models/gnn.py on top of it.
The compute path is the C-ABI library ``_native/libgine_hip.so`` (include/gine_hip.h).
"""
from . import _lib
from .graph import GineGraph, get_graph, graph_cache
from .nn import GINEConv
from .inference import Predictor
from .forecast import Forecast, ForecastScore, TwScore, pit_sample
from .ensemble import EnsembleScore, EnsembleTwScore, RawEnsemble, skill
from .fields import AreaScore, FieldScore, MemberFields
from .importance import (FEATURE_NAMES, FeatureImportance, PermutationPlan, fill_batch,
                         permutation_importance)
from . import compare
from .compare import BootstrapResult, DMResult, PairedScores
from . import reliability
from .reliability import Reliability, ReliabilityBands, ReliabilityFit
from . import pool
from .pool import ForecastPool, PairSums, PoolFit, PoolScore
from . import emos
from .emos import Emos, EmosFit

__all__ = ["AreaScore", "BootstrapResult", "DMResult", "Emos", "EmosFit", "EnsembleScore",
           "EnsembleTwScore",
           "FEATURE_NAMES", "FeatureImportance", "FieldScore", "Forecast", "ForecastPool",
           "ForecastScore",
           "GINEConv", "GineGraph", "MemberFields", "PairSums", "PairedScores", "PermutationPlan",
           "PoolFit", "PoolScore", "Predictor", "RawEnsemble", "Reliability", "ReliabilityBands", "ReliabilityFit",
           "TwScore", "compare", "emos", "fill_batch", "get_graph", "graph_cache", "native_library",
           "permutation_importance", "pit_sample", "pool", "reliability", "skill"]


def native_library():
    """Load (if needed) and return the ctypes handle of libgine_hip.so; raises if missing."""
    return _lib.load()
