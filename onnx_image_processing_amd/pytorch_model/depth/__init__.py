from .depth2pointcloud import DepthToPointCloud
from .depth2pointcloud_with_normal import DepthToPointCloudWithNormal
from .depth_align import DepthAlignment

__all__ = ["DepthToPointCloud", "DepthToPointCloudWithNormal", "DepthAlignment"]
