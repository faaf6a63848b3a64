"""MI355X-native node-relaxation engine for OptimalMatrixCompletion.jl's hot path (HIP, gfx950)."""
from ._lib import LIB_PATH, EXPORTS, OmcError, RelaxParams, load  # noqa: F401
from .api import Engine, default_params, CUT_TYPES, DIR_CODES, BREAKPOINTS, STATUS_NAMES, shor_dual_bound_plan, shor_index_plan  # noqa: F401
from . import data, shor_lists, bnb, bnb_stream, certificate  # noqa: F401,E402
