// feature_hip.h -- the drop-in adapter a maintainer adds to ZhenghaoFei/visual_odom (src/) so that circularMatching(),
// the triangulation pair of main.cpp and trackingFrame2Frame() run on libvo_hip.so (MI355X) instead of OpenCV.
//
//   circularMatching_hip      same signature as circularMatching        feature.h:61-65   (body feature.cpp:118-148)
//   trackingFrame2Frame_hip   same signature as trackingFrame2Frame     visualOdometry.h:36-42 (body visualOdometry.cpp:132-193)
//   triangulate_hip           replaces cv::triangulatePoints + cv::convertPointsFromHomogeneous   main.cpp:169-171
//   detectAndBucket_hip       replaces the head of matchingFeatures     visualOdometry.cpp:95-108
//   featureTracking_hip       same signature as featureTracking         feature.h:52      (body feature.cpp:64-74)
//   featureDetectionGoodFeaturesToTrack_hip   same signature as featureDetectionGoodFeaturesToTrack   feature.h:50 (body feature.cpp:49-62)
//
// Switch: -DUSE_HIP next to the reference's own USE_CUDA (CMakeLists.txt:5-9, visualOdometry.cpp:112-118); see
// adapters/USE_HIP.cmake and INTEGRATION.md.  OpenCV is needed for the TYPES of the existing signatures only (cv::Mat,
// cv::Point2f): no OpenCV algorithm is called.  Where the OpenCV headers are not installed (this repository's test build)
// the same file compiles against a type-only stand-in that the include path provides (oracle/ref_dropin/Makefile:
// -I oracle/ref_shim); oracle/ref_dropin compiles THIS file with the reference's unmodified sources and
// tests/test_gpu_parity.py::test_reference_sources_run_on_libvo_hip runs the result on the GPU; tests/test_gpu_adapter.py calls
// featureTracking_hip, featureDetectionGoodFeaturesToTrack_hip and goodFeaturesToTrack_hip there one by one.
#pragma once

#if __has_include(<opencv2/core.hpp>)
#include <opencv2/core.hpp>   // a machine that has OpenCV: the real cv::Mat / cv::Point2f
#else
#include "vo_cv_shim.h"       // no OpenCV installed: type-only stand-in (test builds of this repository)
#endif

#include <vector>

#include "feature.h"          // FeatureSet (feature.h:33-43), from the reference tree
#include "vo_hip.h"           // C ABI of libvo_hip.so
#include "vo_flow.h"          // ... and its two-image tracker
#include "vo_corners.h"       // ... and its Shi-Tomasi detector
#include "vo_corners_mask.h"  // ... with goodFeaturesToTrack's mask argument
#include "vo_corners_response.h" // ... and its blockSize, useHarrisDetector and k
#include "vo_detector.h"      // ... and the frame loop's choice between FAST and that detector
#include "vo_topup.h"         // ... and that detector's top-up under a mask of the carried points

// same signature as circularMatching (feature.h:61-65)
void circularMatching_hip(cv::Mat img_l_0, cv::Mat img_r_0, cv::Mat img_l_1, cv::Mat img_r_1,
                          std::vector<cv::Point2f>& points_l_0, std::vector<cv::Point2f>& points_r_0,
                          std::vector<cv::Point2f>& points_l_1, std::vector<cv::Point2f>& points_r_1,
                          std::vector<cv::Point2f>& points_l_0_return, FeatureSet& current_features);

// same signature as trackingFrame2Frame (visualOdometry.h:36-42)
void trackingFrame2Frame_hip(cv::Mat& projMatrl, cv::Mat& projMatrr, std::vector<cv::Point2f>& pointsLeft_t0,
                             std::vector<cv::Point2f>& pointsLeft_t1, cv::Mat& points3D_t0, cv::Mat& rotation,
                             cv::Mat& translation, bool mono_rotation = true);

// replaces main.cpp:169-171 (points3D_t0: N x 1 CV_32FC3, what convertPointsFromHomogeneous returns)
void triangulate_hip(cv::Mat& projMatrl, cv::Mat& projMatrr, std::vector<cv::Point2f>& pointsLeft_t0,
                     std::vector<cv::Point2f>& pointsRight_t0, cv::Mat& points3D_t0);

// replaces visualOdometry.cpp:95-108: appendNewFeatures when fewer than 2000 features are carried + bucketingFeatures
// (bucket_size = rows / 10, one feature per bucket: the reference's literals)
void detectAndBucket_hip(cv::Mat& image, FeatureSet& current_features);
// ... with appendNewFeatures' detector call swapped for featureDetectionGoodFeaturesToTrack (feature.cpp:49-62) when
// useGoodFeaturesToTrack is set: carried features, then goodFeaturesToTrack's corners in its own order (vo_detector.h).
// topupRadius >= 0: that call under the disc mask, radius topupRadius, of current_features.points (vo_topup.h); -1: no mask
void detectAndBucket_hip(cv::Mat& image, FeatureSet& current_features, bool useGoodFeaturesToTrack, int topupRadius = -1);

// same signature as featureTracking (feature.h:52): calcOpticalFlowPyrLK(img_1, img_2, ..., 21 x 21, 3, 30 / 0.01, 0, 0.001) +
// deleteUnmatchFeatures.  points1 / points2 come back compacted, status keeps its length (0 also where a tracked point was
// dropped for a negative coordinate), as the reference leaves them.  Drops the pair circularMatching_hip kept, if any.
void featureTracking_hip(cv::Mat img_1, cv::Mat img_2, std::vector<cv::Point2f>& points1, std::vector<cv::Point2f>& points2,
                         std::vector<uchar>& status);

// same signature as featureDetectionGoodFeaturesToTrack (feature.h:50): cv::goodFeaturesToTrack(image, points, 5000, 0.01, 5., Mat(),
// 3, false, 0.04) through vocorn_detect of include/vo_corners.h -- the same corners in the same order.  The reference's frame loop
// never calls it (it detects with FAST); the pair circularMatching_hip kept stays where it is.
void featureDetectionGoodFeaturesToTrack_hip(cv::Mat image, std::vector<cv::Point2f>& points);

// cv::goodFeaturesToTrack(image, points, maxCorners, qualityLevel, minDistance, mask, 3, false, 0.04) through vocmask_detect of
// include/vo_corners_mask.h: mask is empty (no mask) or CV_8UC1 of the image's size, non-zero = allowed -- what a KLT front end
// passes to top its point set up away from the points it still tracks.  maxCorners <= 0: no limit.
void goodFeaturesToTrack_hip(cv::Mat image, std::vector<cv::Point2f>& points, int maxCorners, double qualityLevel, double minDistance, cv::Mat mask);

// ... with upstream's full argument list: cv::goodFeaturesToTrack(image, points, maxCorners, qualityLevel, minDistance, mask, blockSize,
// useHarrisDetector, k) through voresp_detect of include/vo_corners_response.h.  Built: blockSize 3 or 5 (gradientSize stays 3), the
// minimum eigenvalue or the Harris response, any finite k; anything else throws std::runtime_error.
void goodFeaturesToTrack_hip(cv::Mat image, std::vector<cv::Point2f>& points, int maxCorners, double qualityLevel, double minDistance, cv::Mat mask,
                             int blockSize, bool useHarrisDetector, double k);

// OPT-IN, default off: the caller promises that the t0 pair of every circularMatching_hip call IS the t1 pair of the call
// before it -- the reference's loop hands its frames over exactly so (main.cpp:157-158: imageLeft_t0 = imageLeft_t1 shares
// the pixel buffer).  A call whose t0 images have the size, row step and DATA POINTERS of the previous call's t1 images then
// names the pair libvo_hip.so kept on the device with its pyramids (vo_hip.h, THE KEPT PAIR) instead of sending it again:
// two images cross PCIe instead of four and the first hop of the chain starts before they have arrived.  Same results bit
// for bit as long as the promise holds; the pointers only identify the buffer, they cannot see a caller who rewrites it.
// Anything else (first call, other buffers, another user of the context in between: vo_kept_pair_id) sends four images.
void vo_adapter_keep_pair(bool on);
long vo_adapter_kept_calls(); // circularMatching_hip calls that went without their t0 pair so far

// the context the adapter functions share (one per process: the reference is single-threaded), grown to hold a w x h image
// and n points; throws std::runtime_error when there is no HIP device (there is no CPU fallback)
vo_ctx* vo_adapter_context_for(int w, int h, int n);
