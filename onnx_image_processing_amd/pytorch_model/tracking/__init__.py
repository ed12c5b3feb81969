from .feature_tracker import FeatureTracker

__all__ = ["FeatureTracker"]
