from .disparity_filter import DisparityFilter
from .stereo_matcher import StereoMatcher

__all__ = ["StereoMatcher", "DisparityFilter"]
