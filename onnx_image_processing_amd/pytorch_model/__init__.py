"""Drop-in mirrors of the reference's `pytorch_model` sub-packages for the matching hot path.

Same class names, constructor arguments, defaults, ValueErrors, buffer names and forward()
signatures as reference pytorch_model/{detector,utils,descriptor,matching,feature_detection,pointcloud,depth,threshold};
the arithmetic runs in the hand-written gfx950 kernels behind include/mi355x_match.h.
Inputs must be GPU tensors (there is no CPU fallback).  `geometry.relative_pose` and `ingest` have no module in the
reference: they are its hosts' OpenCV steps (pose from matches; colour frame to gray model frame) on the device.
`retrieval` (KeyframeDatabase: which stored keyframe is this frame?) has none either: loop closure detection and
relocalisation are open boxes of the reference's roadmap.  `tracking` (FeatureTracker: pyramidal Lucas-Kanade between two
frames) has none: the reference's hosts call OpenCV for it.  `stereo` (StereoMatcher: a rectified pair to disparity and depth by
census and semi-global matching; DisparityFilter: its speckle and median post-filters) has none either: the reference's OAK-D back
end uses the camera's own stereo engine.
`calibration` (Undistorter, StereoRectifier: lens undistortion and stereo rectification of frames and keypoints) has none: the
reference keeps fx, fy, cx, cy of a camera and drops its distortion coefficients.
"""
