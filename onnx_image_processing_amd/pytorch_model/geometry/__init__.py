from .absolute_pose import AbsolutePoseEstimator
from .bundle_adjustment import BundleAdjuster
from .dense_rgbd import DenseRgbdRefiner
from .direct_rgbd import DirectRgbdRefiner
from .direct_tsdf_volume import DirectTsdfVolume
from .essential_matrix_estimator import EssentialMatrixEstimator
from .landmark_tracks import LandmarkTracks
from .local_map import LocalMapTracker
from .planar_pose import HomographyEstimator, PlanarPoseEstimator, TwoViewPoseEstimator
from .pose_graph import PoseGraphOptimizer
from .relative_pose import RelativePoseEstimator, triangulate_points
from .rgbd_pose import RgbdPoseEstimator
from .similarity import SimilarityEstimator
from .similarity_graph import SimilarityGraphOptimizer
from .tsdf_volume import TsdfVolume

__all__ = ["AbsolutePoseEstimator", "BundleAdjuster", "DenseRgbdRefiner", "DirectRgbdRefiner", "DirectTsdfVolume", "EssentialMatrixEstimator", "HomographyEstimator",
           "LandmarkTracks", "LocalMapTracker", "PlanarPoseEstimator", "PoseGraphOptimizer", "RelativePoseEstimator", "RgbdPoseEstimator", "SimilarityEstimator", "SimilarityGraphOptimizer", "TsdfVolume", "TwoViewPoseEstimator", "triangulate_points"]
