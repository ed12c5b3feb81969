from .frame_ingest import FrameIngest, scale_intrinsics

__all__ = ["FrameIngest", "scale_intrinsics"]
