from .trajectory_check import TrajectoryChecker, TrajectoryCheckResult  # noqa: F401
