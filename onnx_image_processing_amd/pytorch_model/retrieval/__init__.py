from .keyframe_database import KeyframeDatabase

__all__ = ["KeyframeDatabase"]
