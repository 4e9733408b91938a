from .trajectory_check import TrajectoryChecker, TrajectoryCheckResult  # noqa: F401
from .ensemble_check import EnsembleChecker, EnsembleCheckResult  # noqa: F401
from .clearance import ClearanceQuery, ClearanceResult  # noqa: F401
from .trajectory_score import TrajectoryScorer, TrajectoryScoreResult  # noqa: F401
from .lift import TrajectoryLifter, TrajectoryLiftResult  # noqa: F401
from .pick import TrajectoryPicker, TrajectoryPickResult  # noqa: F401
from .ensemble_pick import EnsemblePicker, EnsemblePickResult  # noqa: F401
