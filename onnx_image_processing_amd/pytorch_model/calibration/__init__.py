from .rectification import StereoRectifier, Undistorter

__all__ = ["Undistorter", "StereoRectifier"]
