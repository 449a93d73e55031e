"""linear_programming_solver_amd — MI355X-native dense simplex pivot engine.

Host-side mirror of the reference's operator interface for ONE path (the simplex pivot loop), over the
C ABI of liblpx.so (include/lpx.h): LPStandardForm, LPState {get_entering, get_leaving, pivot},
LPSolver.solve, LPInputReader; LPBatch / LPSolver.solve_batch for many small LPs in one launch; LPScenarios /
LPSolver.solve_scenarios for many (b, c) on one matrix.  There is no CPU fallback: without the HIP library every compute call raises.
"""
from ._lib import set_default_arithmetic  # noqa: F401
from .errors import LPException, SolutionException  # noqa: F401
from .lp_batch import LPBatch, pack_lps  # noqa: F401
from .lp_input_reader import LPInputReader  # noqa: F401
from .lp_multi import LPMulti  # noqa: F401
from .lp_scenarios import LPScenarios  # noqa: F401
from .lp_solver import LPSolver  # noqa: F401
from .lp_standard_form import LPStandardForm  # noqa: F401
from .lp_state import LPState  # noqa: F401

__all__ = ["LPException", "SolutionException", "LPBatch", "pack_lps", "LPInputReader", "LPMulti", "LPScenarios", "LPSolver", "LPStandardForm", "LPState",
           "set_default_arithmetic"]
