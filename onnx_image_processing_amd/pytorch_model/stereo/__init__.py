from .stereo_matcher import StereoMatcher

__all__ = ["StereoMatcher"]
