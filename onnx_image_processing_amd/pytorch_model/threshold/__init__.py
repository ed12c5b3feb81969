from .otsu import OtsuThreshold
from .multi_otsu import MultiOtsuThreshold

__all__ = ["OtsuThreshold", "MultiOtsuThreshold"]
