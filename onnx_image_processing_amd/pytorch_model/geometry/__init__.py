from .essential_matrix_estimator import EssentialMatrixEstimator
from .relative_pose import RelativePoseEstimator, triangulate_points

__all__ = ["EssentialMatrixEstimator", "RelativePoseEstimator", "triangulate_points"]
