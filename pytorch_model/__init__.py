"""`pytorch_model` -- the reference's top-level package name, as an alias of onnx_image_processing_amd.pytorch_model.

With the repository root on sys.path, the reference's own import lines work unchanged and resolve to the
MI355X implementation (the very same module objects, not copies):

    from pytorch_model.detector import ShiTomasiScore
    from pytorch_model.descriptor.bad import SparseBAD
    from pytorch_model.matching.outlier_filters import probability_ratio_filter
    from pytorch_model.feature_detection.shi_tomasi_sparse_bad_sinkhorn import ShiTomasiSparseBADSinkhornMatcher
    from pytorch_model.pointcloud.voxel_downsampling import VoxelDownsampling
    from pytorch_model.depth.depth2pointcloud import DepthToPointCloud
    from pytorch_model.depth.depth_align import DepthAlignment
    from pytorch_model.threshold.otsu import OtsuThreshold
    from pytorch_model.threshold.multi_otsu import MultiOtsuThreshold
    from pytorch_model.ingest import FrameIngest, scale_intrinsics      (no counterpart in the reference: its hosts' CPU step)
    from pytorch_model.retrieval import KeyframeDatabase                (no counterpart in the reference: its roadmap's loop closure)
    from pytorch_model.geometry import PoseGraphOptimizer               (no counterpart in the reference: closes the loop found)
    from pytorch_model.geometry import LandmarkTracks                   (no counterpart in the reference: matches -> BA windows)
    from pytorch_model.geometry import LocalMapTracker                  (no counterpart in the reference: landmarks -> a new frame)
    from pytorch_model.geometry import SimilarityEstimator              (no counterpart in the reference: Sim(3) between two maps)
    from pytorch_model.geometry import SimilarityGraphOptimizer         (no counterpart in the reference: 7-DoF loop closing)
    from pytorch_model.tracking import FeatureTracker                   (no counterpart in the reference: KLT tracking, its hosts' cv2 step)
    from pytorch_model.stereo import StereoMatcher                      (no counterpart in the reference: a stereo rig's depth, cv2.StereoSGBM)
    from pytorch_model.stereo import DisparityFilter                    (no counterpart in the reference: cv2.filterSpeckles, cv2.medianBlur on disparities)
    from pytorch_model.calibration import Undistorter, StereoRectifier  (no counterpart in the reference: cv2.remap, cv2.undistortPoints, cv2.stereoRectify)

The one sub-package outside the mirrored set (`vo`, host-side numpy / OpenCV and camera drivers) does not
exist and raises ImportError.
"""
import importlib
import importlib.abc
import importlib.util
import sys

_IMPL = "onnx_image_processing_amd.pytorch_model"


class _AliasFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path=None, target=None):
        if not name.startswith(__name__ + "."):
            return None
        real = _IMPL + name[len(__name__):]
        try:
            importlib.import_module(real)
        except ImportError:
            return None
        return importlib.util.spec_from_loader(name, self, is_package=hasattr(sys.modules[real], "__path__"))

    def create_module(self, spec):
        return sys.modules[_IMPL + spec.name[len(__name__):]]

    def exec_module(self, module):
        pass


if not any(isinstance(f, _AliasFinder) for f in sys.meta_path):
    sys.meta_path.insert(0, _AliasFinder())
_impl = importlib.import_module(_IMPL)
__doc__ = (__doc__ or "") + "\n" + (_impl.__doc__ or "")
