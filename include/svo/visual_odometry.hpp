// visual_odometry.hpp — header-only C++ facade over the C-ABI (include/svo.h) that mirrors the
// reference's C++ surface, namespace visual_odometry (reference include/vo.h:46-472): same class and
// function names, same argument order and meaning, same failure behaviour.  Only the OpenCV types
// are substituted: cv::Mat (8-bit image) -> Image, cv::Point2f -> Point2f, cv::Mat_<float> 3x4 ->
// Mat34f, cv::Mat_<double> 4x4 -> Mat44, cv::Mat inliers (Nx1 int32) -> std::vector<int>.
// Link with -lsvo_hip.  All arithmetic runs on the GPU; errors surface as std::runtime_error with
// svo_last_error() (the reference would surface cv::Exception).
#pragma once
#include <array>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "../svo.h"

namespace visual_odometry {

// the reference's constants (include/vo.h:53-127)
const int BUCKET_START_ROW = 4;
const int BUCKETS_ALONG_HEIGHT = 92;
const int BUCKETS_ALONG_WIDTH = 160;
const int FEATURES_PER_BUCKET = 1;
const int FEATURES_THRESHOLD = 15;
const int PRE_MATCHING_FEATURE_THRESHOLD = 100;
const int AGE_THRESHOLD = 20;
const int FAST_THRESHOLD = 20;
const float RANSAC_REPROJECTION_ERROR = 8;
const int RANSAC_ITERATIONS = 100;
const double OPTICAL_FLOW_MIN_EIG_THRESHOLD = 0.001;
const double CIRCULAR_MATCHING_SUCCESS_THRESHOLD = .15;
const double MAX_TRANSLATION_NORM = .1;
const double MAX_ROTATION_NORM = .5;

struct Point2f { float x, y; };
struct Point3f { float x, y, z; };
using Mat34f = std::array<float, 12>;     // 3x4 row-major
using Mat33f = std::array<float, 9>;
using Mat33d = std::array<double, 9>;
using Vec3d = std::array<double, 3>;
using Mat44 = std::array<double, 16>;     // 4x4 row-major

// 8-bit single-channel image view (what cv_bridge MONO8 delivers, reference src/stereo_vo.cpp:9)
struct Image {                                                        // the part of cv::Mat the path uses: 8-bit, 1 or 3 channels
    const uint8_t* data = nullptr;
    int rows = 0, cols = 0, step = 0;                                 // step in bytes
    int channels = 1;                                                 // 3 = interleaved BGR, as cv::imread returns it (main.cpp:38-39);
                                                                      // with VisualOdometry::set_input_encoding: the encoding's bytes per pixel
    Image() {}
    Image(const uint8_t* d, int r, int c, int s = 0, int cn = 1) : data(d), rows(r), cols(c), step(s ? s : c * cn), channels(cn) {}
    bool empty() const { return !data || rows <= 0 || cols <= 0; }
};

inline void svo_throw(int rc) { if (rc < 0) throw std::runtime_error(std::string("libsvo_hip: ") + svo_last_error()); }
inline int& default_device() { static int d = 0; return d; }

class FeatureSet {                                                   // include/vo.h:132-188
   public:
    std::vector<Point2f> points;
    std::vector<int> ages;
    std::vector<int> strengths;
    int size() { return (int)points.size(); }
    void clear() { points.clear(); ages.clear(); strengths.clear(); }
    void filterByBucketLocationInternal(const Image& image, const int buckets_along_height, const int buckets_along_width,
                                        const int bucket_start_row, const int features_per_bucket) {
        int n = size();
        svo_throw(svo_bucket_filter(default_device(), image.cols, image.rows, &n, n ? &points[0].x : nullptr,
                                    n ? ages.data() : nullptr, n ? strengths.data() : nullptr, buckets_along_height,
                                    buckets_along_width, bucket_start_row, features_per_bucket, AGE_THRESHOLD, FAST_THRESHOLD));
        points.resize(n); ages.resize(n); strengths.resize(n);
    }
    void filterByBucketLocation(const Image& image) {
        filterByBucketLocationInternal(image, BUCKETS_ALONG_HEIGHT, BUCKETS_ALONG_WIDTH, BUCKET_START_ROW, FEATURES_PER_BUCKET);
    }
    void appendFeaturesFromImage(const Image& image, const int fast_threshold) {
        int n = size();
        int cap = (BUCKETS_ALONG_HEIGHT - BUCKET_START_ROW) * BUCKETS_ALONG_WIDTH;
        if (cap < n) cap = n;
        points.resize(cap); ages.resize(cap); strengths.resize(cap);
        svo_throw(svo_append_features_from_image(default_device(), nullptr, image.data, image.cols, image.rows, image.step,
                                                 fast_threshold, cap, &n, &points[0].x, ages.data(), strengths.data()));
        points.resize(n); ages.resize(n); strengths.resize(n);
    }
};

class Bucket {                                                       // include/vo.h:195-229
   public:
    int max_size;
    FeatureSet features;
    Bucket(int max_size_) : max_size(max_size_) {}
    int compute_score(const int age, const int strength) { return age + (strength - FAST_THRESHOLD) / 20; }
    void add_feature(const Point2f point, const int age, const int strength) {
        // the insertion rule (feature_set.cpp:20-53) runs on the GPU: the bucket's current content, in slot order, followed by
        // the new feature goes through a 1x1 grid of this capacity — the stored features refill their slots in the same order
        // (they passed the age test when they entered), then the new one meets exactly the state the reference's bucket is in.
        // One call with at most max_size + 1 inputs per insertion (not a replay of everything ever offered).
        if (!max_size) return;
        features.points.push_back(point); features.ages.push_back(age); features.strengths.push_back(strength);
        float mx = 1;
        for (auto& p : features.points) { if (p.x > mx) mx = p.x; if (p.y > mx) mx = p.y; }
        Image dims(reinterpret_cast<const uint8_t*>(this), (int)mx + 2, (int)mx + 2);   // only rows/cols are read
        features.filterByBucketLocationInternal(dims, 1, 1, 0, max_size);
    }
    int size() { return features.size(); }
};

// the body of both forms of featureDetectionFast (not part of the reference's surface): detect into room for `cap` keypoints, again
// with more room when there were more; mask null: no mask
inline std::vector<Point2f> fast_detect_all(const Image& image, const uint8_t* mask, int mask_step, int fast_threshold,
                                            std::vector<float>& response_strengths) {
    int cap = 8192, n = 0;
    std::vector<Point2f> pts;
    for (;;) {
        pts.resize(cap); response_strengths.resize(cap);
        svo_throw(mask ? svo_fast_detect_masked(default_device(), image.data, image.cols, image.rows, image.step, fast_threshold,
                                                mask, mask_step, cap, &pts[0].x, response_strengths.data(), &n)
                       : svo_fast_detect(default_device(), image.data, image.cols, image.rows, image.step, fast_threshold, cap,
                                         &pts[0].x, response_strengths.data(), &n));
        if (n <= cap) break;
        cap = n;
    }
    pts.resize(n); response_strengths.resize(n);
    return pts;
}

inline std::vector<Point2f> featureDetectionFast(const Image image, const int fast_threshold,
                                                 std::vector<float>& response_strengths) {          // vo.h:393-395
    return fast_detect_all(image, nullptr, 0, fast_threshold, response_strengths);
}

// the same behind a detection mask (svo.h: an 8-bit image of the frame's size, non-zero = features allowed, applied to the keypoints
// that survived non-max suppression — what cv::FeatureDetector::detect(image, keypoints, mask) does)
inline std::vector<Point2f> featureDetectionFast(const Image image, const Image mask, const int fast_threshold,
                                                 std::vector<float>& response_strengths) {
    if (mask.empty() || mask.rows != image.rows || mask.cols != image.cols || mask.channels != 1)
        throw std::runtime_error("featureDetectionFast: the mask must be a single-channel image of the frame's size");
    return fast_detect_all(image, mask.data, mask.step, fast_threshold, response_strengths);
}

inline void deletePointsWithFailureStatus(std::vector<Point2f>& point_vector, const std::vector<bool>& isok) {   // vo.h:406-407
    size_t m = 0;
    for (size_t i = 0; i < point_vector.size(); i++)
        if (i >= isok.size() || isok[i]) point_vector[m++] = point_vector[i];
    point_vector.resize(m);
}

inline void deleteFeaturesWithFailureStatus(FeatureSet& f, const std::vector<bool>& isok) {                    // vo.h:416-417
    size_t m = 0;
    for (size_t i = 0; i < f.points.size(); i++)
        if (i >= isok.size() || isok[i]) { f.points[m] = f.points[i]; f.ages[m] = f.ages[i]; f.strengths[m] = f.strengths[i]; m++; }
    f.points.resize(m); f.ages.resize(m); f.strengths.resize(m);
}

inline std::vector<bool> findClosePoints(const std::vector<Point2f>& points_1, const std::vector<Point2f>& points_2,
                                         float threshold) {                                                     // vo.h:430-432
    std::vector<uint8_t> ok(points_1.size());
    if (!points_1.empty())
        svo_throw(svo_find_close_points(default_device(), (int)points_1.size(), &points_1[0].x, &points_2[0].x, threshold, ok.data()));
    return std::vector<bool>(ok.begin(), ok.end());
}

// vo.h:452-456.  rotation (3x3) and translation (3) are in/out exactly as in the reference.
inline std::pair<std::vector<int>, bool> cameraToWorld(const Mat33f& cameraProjection, const std::vector<Point2f>& cameraPoints,
                                                       const std::vector<Point3f>& worldPoints, Mat33d& rotation, Vec3d& translation) {
    int n = (int)cameraPoints.size(), nin = 0, ok = 0;
    std::vector<int> inl(n > 0 ? n : 1);
    svo_throw(svo_camera_to_world(default_device(), cameraProjection.data(), n, n ? &cameraPoints[0].x : nullptr,
                                  n ? &worldPoints[0].x : nullptr, rotation.data(), translation.data(), inl.data(), &nin, &ok,
                                  RANSAC_ITERATIONS, RANSAC_REPROJECTION_ERROR, 0.98f, nullptr));
    inl.resize(nin);
    return std::make_pair(inl, ok != 0);
}

inline Mat44 getInverseTransform(const Mat33d& rotation, const Vec3d& translation_stereo) {                     // vo.h:469-470
    Mat44 T;
    svo_throw(svo_inverse_transform(default_device(), rotation.data(), translation_stereo.data(), T.data()));
    return T;
}

class VisualOdometry {                                               // include/vo.h:231-380
   public:
    // vo.h:273.  Like the reference, a first frame needs no projection matrices (vo.cpp:47-56 only caches); until
    // initalize_projection_matricies is called they are all-zero, as the reference's empty Mats effectively are
    Mat34f leftCameraProjection_{}, rightCameraProjection_{};
    VisualOdometry() { svo_config_default(&cfg_); }
    explicit VisualOdometry(const svo_config& cfg) : cfg_(cfg) {}
    // the 2-argument form src/stereo_vo.cpp:50 calls (missing from the reference's own header)
    VisualOdometry(const Mat34f& Pl, const Mat34f& Pr) { svo_config_default(&cfg_); initalize_projection_matricies(Pl, Pr); }
    ~VisualOdometry() { svo_destroy(ctx_); }
    VisualOdometry(const VisualOdometry&) = delete;
    VisualOdometry& operator=(const VisualOdometry&) = delete;

    void initalize_projection_matricies(const Mat34f leftCameraProjection, const Mat34f rightCameraProjection) {   // vo.h:307-309
        leftCameraProjection_ = leftCameraProjection; rightCameraProjection_ = rightCameraProjection;
        if (ctx_) svo_throw(svo_set_projection(ctx_, -1, leftCameraProjection_.data(), rightCameraProjection_.data()));
    }

    // vo.h:333-334: (success, transform).  On failure the transform is the last successful one (identity at first).
    std::pair<bool, Mat44> stereo_callback(const Image& image_left, const Image& image_right) {
        if (image_left.empty() || image_right.empty()) throw std::runtime_error("stereo_callback: empty image");
        if (image_left.channels != image_right.channels) throw std::runtime_error("stereo_callback: channel mismatch");
        if (!ctx_) first_frame(image_left);
        check_frame(image_left, "left"); check_frame(image_right, "right");
        Mat44 T;
        int rc = svo_process(ctx_, image_left.data, image_right.data, image_left.step, T.data(), &stats);
        svo_throw(rc);
        return std::make_pair(rc == 1, T);
    }
    // vo.h:374-379, vo.cpp:169-240.  Tracks pointsLeftT0 around the loop T0-left -> T1-left -> T1-right -> T0-right -> T0-left,
    // removes every point (and its feature) that lost an LK status or does not close the loop within 0.15 px, and makes the
    // T1 pyramids the cached pair (vo.cpp:231-232; on empty input it returns before doing so, :179-181).  As in the
    // reference this is a member call on the SAME state stereo_callback works on: the T0 side is the pyramid pair cached on
    // the device by the previous stereo_callback / circularMatching (prime it with stereo_callback, as main.cpp:191 does), and
    // the next stereo_callback tracks against the pair cached here.
    void circularMatching(const Image& imgLeftT1, const Image& imgRightT1, std::vector<Point2f>& pointsLeftT0,
                          std::vector<Point2f>& pointsRightT0, std::vector<Point2f>& pointsLeftT1,
                          std::vector<Point2f>& pointsRightT1, FeatureSet& current_features) {
        if (pointsLeftT0.empty()) return;                                                          // vo.cpp:179-181
        if (!ctx_) throw std::runtime_error("circularMatching: no cached pyramids (call stereo_callback first)");
        check_frame(imgLeftT1, "left"); check_frame(imgRightT1, "right");
        const int n = (int)pointsLeftT0.size();
        std::vector<Point2f> loop(n);
        std::vector<uint8_t> ok(n);
        pointsLeftT1.resize(n); pointsRightT1.resize(n); pointsRightT0.resize(n);
        svo_throw(svo_circular_matching(ctx_, imgLeftT1.data, imgRightT1.data, imgLeftT1.step, n, &pointsLeftT0[0].x, &pointsLeftT1[0].x,
                                        &pointsRightT1[0].x, &pointsRightT0[0].x, &loop[0].x, ok.data()));
        const std::vector<bool> keep(ok.begin(), ok.end());
        deleteFeaturesWithFailureStatus(current_features, keep);                                    // vo.cpp:233
        deletePointsWithFailureStatus(pointsLeftT0, keep); deletePointsWithFailureStatus(pointsLeftT1, keep);   // :234-238
        deletePointsWithFailureStatus(pointsRightT0, keep); deletePointsWithFailureStatus(pointsRightT1, keep);
    }

    // vo.h:354-362, vo.cpp:315-366: detect on imageLeftT0 (second pass at threshold / 4 if fewer than 100 features), track the
    // feature set through circularMatching, then drop everything that left the image in any of the four views.
    // As in the reference, imageLeftT0 is only what FAST runs on (vo.cpp:325); the loop's T0 side is the cached pyramid pair
    // (imageRightT0 is not read at all, vo.cpp:315-366), so the caller primes the object with stereo_callback(imageLeftT0, imageRightT0).
    void matchingFeatures(const Image& imageLeftT0, const Image& imageRightT0, const Image& imageLeftT1, const Image& imageRightT1,
                          FeatureSet& currentVOFeatures, std::vector<Point2f>& pointsLeftT0, std::vector<Point2f>& pointsRightT0,
                          std::vector<Point2f>& pointsLeftT1, std::vector<Point2f>& pointsRightT1) {
        currentVOFeatures.appendFeaturesFromImage(imageLeftT0, FAST_THRESHOLD);                     // vo.cpp:325
        if (currentVOFeatures.size() < PRE_MATCHING_FEATURE_THRESHOLD)                              // :327-332
            currentVOFeatures.appendFeaturesFromImage(imageLeftT0, FAST_THRESHOLD / 4);
        pointsLeftT0 = currentVOFeatures.points;                                                    // :338
        (void)imageRightT0;
        circularMatching(imageLeftT1, imageRightT1, pointsLeftT0, pointsRightT0, pointsLeftT1, pointsRightT1, currentVOFeatures);
        std::vector<bool> inside(pointsLeftT0.size());                                              // :341-359
        for (size_t i = 0; i < inside.size(); i++) {
            const Point2f* q[4] = {&pointsLeftT0[i], &pointsLeftT1[i], &pointsRightT0[i], &pointsRightT1[i]};
            bool in = true;
            for (const Point2f* p : q) if (p->x < 0 || p->y < 0 || p->y >= height_ || p->x >= width_) in = false;   // the (rectified) image size
            inside[i] = in;
        }
        deleteFeaturesWithFailureStatus(currentVOFeatures, inside);                                 // :360-364
        deletePointsWithFailureStatus(pointsLeftT0, inside); deletePointsWithFailureStatus(pointsLeftT1, inside);
        deletePointsWithFailureStatus(pointsRightT0, inside); deletePointsWithFailureStatus(pointsRightT1, inside);
    }

    // Start over as a freshly constructed object with the same projection matrices: the next stereo_callback is a first frame
    // (svo_reset_sequence).  The reference has no counterpart; there a tracker that is lost is replaced by a new VisualOdometry.
    void reset() {
        if (ctx_) svo_throw(svo_reset_sequence(ctx_, 0, nullptr, nullptr));
    }

    // Rectify raw frames on the GPU (svo_set_rectification; replaces image_geometry::PinholeCameraModel::rectifyImage, i.e.
    // cv::initUndistortRectifyMap + cv::remap, what stereo_image_proc runs to publish image_rect).  From then on stereo_callback /
    // circularMatching take RAW frames of left.width x left.height; the rectified size is the object's (learnt from the first
    // frame when the call comes before it: then the raw size, as image_rect has).  Projection matrices are not touched: pass
    // left.P / right.P to initalize_projection_matricies.  Takes effect from the next frame.
    void set_rectification(const svo_camera_info& left, const svo_camera_info& right) {
        if (ctx_) svo_throw(svo_set_rectification(ctx_, -1, &left, &right));
        held_.rect_l = left; held_.rect_r = right; held_.rect = true;
    }
    void clear_rectification() {                                     // back to rectified input (svo_clear_rectification)
        held_.rect = false;
        if (ctx_) svo_throw(svo_clear_rectification(ctx_));
    }

    // The sensor_msgs encoding of the frames passed from now on (svo_set_input_format; replaces cv_bridge::toCvCopy(img, MONO8),
    // stereo_vo.cpp:6-14): "mono8", "bgr8", "rgb8", "bgra8", "rgba8", "yuv422" (UYVY), "yuv422_yuy2".  The conversion to grey runs
    // on the GPU inside frame ingest (before rectification); Image::channels is then the encoding's bytes per pixel.  Single-channel
    // objects only; an unknown name throws.  Takes effect from the next frame.
    void set_input_encoding(const char* encoding) {
        static const struct { const char* name; int format; } table[] = {
            {"mono8", SVO_INPUT_MONO8}, {"bgr8", SVO_INPUT_BGR8}, {"rgb8", SVO_INPUT_RGB8}, {"bgra8", SVO_INPUT_BGRA8},
            {"rgba8", SVO_INPUT_RGBA8}, {"yuv422", SVO_INPUT_UYVY}, {"yuv422_yuy2", SVO_INPUT_YUY2}};
        int format = -1;
        for (const auto& e : table) if (encoding && !std::strcmp(encoding, e.name)) format = e.format;
        if (format < 0) throw std::runtime_error(std::string("set_input_encoding: unknown encoding ") + (encoding ? encoding : "(null)"));
        if (ctx_) svo_throw(svo_set_input_format(ctx_, format));
        held_.in_format = format;
    }

    // A 6x6 covariance with every pose from the next frame on (svo_set_pose_covariance): mode SVO_COV_RESIDUAL (sigma^2 from the
    // frame's own reprojection residuals), SVO_COV_FIXED_SIGMA (sigma = pixel_sigma pixels) or SVO_COV_OFF.  A bad mode or sigma throws.
    void set_pose_covariance(int mode, double pixel_sigma = 1.0) {
        if (ctx_) svo_throw(svo_set_pose_covariance(ctx_, mode, pixel_sigma));
        else check_cov(mode, pixel_sigma);
        held_.cov_mode = mode; held_.cov_sigma = pixel_sigma;
    }
    // Equalise both images of every frame passed from now on (svo_set_clahe; replaces cv::createCLAHE(clip, Size(tx, ty))->apply()
    // on the caller's CPU): on the grey frame, after set_input_encoding's conversion and before rectification.  tx, ty: 1 .. 16.
    // Before the first frame the setting is kept and applied when the context is created; bad tiles or a non-finite clip throw at once.
    void set_clahe(double clip = 2.0, int tx = 8, int ty = 8) {
        if (ctx_) svo_throw(svo_set_clahe(ctx_, 1, clip, tx, ty));
        else check_clahe(clip, tx, ty);
        held_.clahe_on = true; held_.clahe_clip = clip; held_.clahe_tx = tx; held_.clahe_ty = ty;
    }
    void clear_clahe() {
        held_.clahe_on = false;
        if (ctx_) svo_throw(svo_set_clahe(ctx_, 0, 0., 0, 0));
    }
    // Keep features off the zero bytes of `mask` (svo_set_detection_mask): height rows of width bytes, `stride` apart (0: packed), at
    // the frame's size (the rectified size of a rectifying object).  The mask describes the left image of the frames passed from
    // now on and is applied when that image is scanned, in the following call; a static mask is set once.  Before the first frame
    // the object keeps a copy (width x height then come from set_detection_mask's own arguments).
    void set_detection_mask(const uint8_t* mask, int stride = 0) {
        if (!mask) { clear_detection_mask(); return; }
        if (!ctx_) throw std::runtime_error("set_detection_mask: before the first frame, pass the size too: set_detection_mask(mask, stride, width, height)");
        svo_throw(svo_set_detection_mask(ctx_, -1, mask, stride ? stride : width_, 0));
    }
    void set_detection_mask(const uint8_t* mask, int stride, int width, int height) {
        if (ctx_) {
            if (width != width_ || height != height_) throw std::runtime_error("set_detection_mask: the mask is not of the frame's size");
            set_detection_mask(mask, stride);
            return;
        }
        if (!mask || width < 1 || height < 1 || (stride && stride < width)) throw std::runtime_error("set_detection_mask: bad arguments");
        held_.mask.resize((size_t)width * height);
        for (int y = 0; y < height; y++) std::memcpy(held_.mask.data() + (size_t)y * width, mask + (size_t)y * (stride ? stride : width), (size_t)width);
    }
    void clear_detection_mask() {
        held_.mask.clear();
        if (ctx_) svo_throw(svo_set_detection_mask(ctx_, -1, nullptr, 0, 0));
    }
    // Of the last stereo_callback (svo_get_last_pose_covariance): cov_T, the covariance of the returned transform in the order
    // (x y z, rotation about x y z) of nav_msgs/Odometry.pose.covariance, and cov_p, that of the cameraToWorld parameters (r, t);
    // both row-major 6x6, all zero with valid = false when the frame gave no pose.  Throws when the frame ran with the mode off.
    struct PoseCovariance { std::array<double, 36> cov_T, cov_p; bool valid; };
    PoseCovariance last_pose_covariance() const {
        PoseCovariance c; int valid = 0;
        svo_throw(svo_get_last_pose_covariance(need_frame("last_pose_covariance"), c.cov_T.data(), c.cov_p.data(), &valid));
        c.valid = valid != 0;
        return c;
    }

    // Persistent feature ids and per-frame stereo observations for a landmark back end (svo_set_track_output): from the next frame
    // on every stereo_callback leaves up to max_rows rows of svo_track_obs — (id, the track's four points, its triangulated point,
    // age, flags), svo.h states the identity rule — read with last_track_observations().  Before the first frame the setting is
    // kept and applied when the context is created; max_rows < 1 throws at once.
    void set_track_output(int max_rows) {
        if (ctx_) svo_throw(svo_set_track_output(ctx_, 1, max_rows));
        else if (max_rows < 1) throw std::runtime_error("set_track_output: max_rows must be >= 1");
        held_.track_rows = max_rows;
    }
    void clear_track_output() {
        held_.track_rows = 0; held_.desc_on = false;                            // the descriptors ride on the track output
        if (ctx_) svo_throw(svo_set_track_output(ctx_, 0, 0));
    }
    // The rows of the last stereo_callback, the first min(tracks, max_rows) in svo_get_last_tracks' order; host memory only.
    // Throws when that frame ran with the output off.
    std::vector<svo_track_obs> last_track_observations() const {
        return last_rows<svo_track_obs>("last_track_observations", svo_get_last_track_obs);
    }

    // A 32-byte binary descriptor beside every observation row (svo_set_descriptor_output; svo.h defines it: a steered BRIEF-256 of
    // the library's own, not cv::ORB's): needs set_track_output first, goes off with it.  Before the first frame the setting is kept
    // and applied, behind the track output, when the context is created.
    void set_descriptor_output(bool on) {
        if (ctx_) svo_throw(svo_set_descriptor_output(ctx_, on ? 1 : 0));
        else if (on && held_.track_rows < 1) throw std::runtime_error("set_descriptor_output: the track output is off (set_track_output first)");
        held_.desc_on = on;
    }
    // The descriptors of the last stereo_callback: 32 bytes per row, row i describes last_track_observations()[i]; host memory only.
    // Throws when that frame ran with descriptors off.
    std::vector<std::array<uint8_t, SVO_DESC_BYTES>> last_track_descriptors() const {
        return last_rows<std::array<uint8_t, SVO_DESC_BYTES>>("last_track_descriptors", svo_get_last_track_descriptors);
    }

    // Seed the temporal LK passes of the NEXT stereo_callback with a predicted flow (svo_set_motion_prior; OpenCV's
    // OPTFLOW_USE_INITIAL_FLOW, which the reference does not use): H (3x3 row-major f32) maps pixels of the previous frame to
    // predicted pixels of the next one; Hi is its inverse, nullptr: the library inverts H.  One-shot: consumed by that frame.
    // H = nullptr clears a pending prior.  Needs the context, i.e. a first frame: before it there is no previous frame to predict from.
    void set_motion_prior(const float* H, const float* Hi = nullptr) {
        svo_throw(svo_set_motion_prior(need_frame("set_motion_prior", "the prior predicts from the previous frame"), 0, H, Hi));
    }
    // The same from a rotation (svo_motion_prior_from_rotation): R (3x3 row-major f64) rotates T0-camera coordinates into T1-camera
    // coordinates — a gyro's integrated increment moved into the camera frame; K is the left projection matrix's.
    void set_rotation_prior(const double* R) {
        float H[9], Hi[9];
        svo_throw(svo_motion_prior_from_rotation(leftCameraProjection_.data(), R, H, Hi));
        set_motion_prior(H, Hi);
    }
    // Without a gyro: SVO_PRIOR_LAST_ROTATION makes every stereo_callback that has no explicit prior predict one on the device from
    // the rotation of the last frame, when that frame gave a pose (svo_set_motion_prior_mode; svo.h has the rule).  Before the first
    // frame the mode is kept and applied when the context is created; an unknown mode throws at once.
    void set_motion_prior_mode(int mode) {
        if (mode != SVO_PRIOR_EXPLICIT && mode != SVO_PRIOR_LAST_ROTATION) throw std::runtime_error("set_motion_prior_mode: unknown mode");
        if (ctx_) svo_throw(svo_set_motion_prior_mode(ctx_, mode));
        held_.prior_mode = mode;
    }
    // What the last stereo_callback used (svo_get_last_motion_prior): source 0 none, 1 explicit, 2 predicted; H, Hi valid when != 0.
    struct MotionPrior { std::array<float, 9> H, Hi; int source; };
    MotionPrior last_motion_prior() const {
        MotionPrior p{};
        svo_throw(svo_get_last_motion_prior(need_frame("last_motion_prior"), 0, p.H.data(), p.Hi.data(), &p.source));
        return p;
    }

    // functor form for boost::bind / message_filters style registration (src/stereo_vo.cpp:61-62)
    void operator()(const Image& l, const Image& r) { stereo_callback(l, r); }

    svo_frame_stats stats{};                                          // the counters the reference printf's (vo.cpp:226..365)
    svo_context* handle() { return ctx_; }

   private:
    // cv::Mat carries its own size and type and OpenCV asserts on mismatches; raw pointers do not, so the facade checks every
    // frame against the context (a shorter or narrower buffer would be read past its end)
    void check_frame(const Image& im, const char* which) const {
        if (im.empty()) throw std::runtime_error(std::string(which) + " image is empty");
        const int w = held_.rect ? held_.rect_l.width : width_, h = held_.rect ? held_.rect_l.height : height_;   // rectifying: frames are raw
        static const int bytes_per_pixel[7] = {1, 3, 3, 4, 4, 2, 2};              // of SVO_INPUT_*
        const int cn = held_.in_format != SVO_INPUT_MONO8 ? bytes_per_pixel[held_.in_format] : cfg_.channels;
        if (im.cols != w || im.rows != h || im.channels != cn || im.step < im.cols * im.channels)
            throw std::runtime_error(std::string(which) + " image does not match the size / channels the object takes (the raw size when rectifying)");
    }
    friend class DescriptorIndex;                                     // (need_frame)
    // the context, once a frame has created it
    svo_context* need_frame(const char* what, const char* why = "call stereo_callback first") const {
        if (!ctx_) throw std::runtime_error(std::string(what) + ": no frame yet (" + why + ")");
        return ctx_;
    }
    // the rows of the last stereo_callback through a (ctx, seq, cap, rows, n_tracks) getter: sized by a first call, filled by a second
    template <class Row, class Elem>
    std::vector<Row> last_rows(const char* what, int (*get)(svo_context*, int, int, Elem*, int*)) const {
        svo_context* ctx = need_frame(what);
        int n_tracks = 0;
        svo_throw(get(ctx, 0, 0, nullptr, &n_tracks));
        std::vector<Row> rows((size_t)(n_tracks > 0 ? n_tracks : 0));
        const int n = get(ctx, 0, (int)rows.size(), rows.empty() ? nullptr : reinterpret_cast<Elem*>(rows.data()), nullptr);
        svo_throw(n);
        rows.resize((size_t)n);
        return rows;
    }

    // What the setters asked for ("Facades: settings before the first frame"): held until the first frame creates the
    // context, and kept current afterwards (check_frame reads in_format).  The projection matrices are the public members above.
    struct Held {
        bool rect = false; svo_camera_info rect_l{}, rect_r{};        // set_rectification: frames are then raw, rect_l.width x rect_l.height
        int in_format = SVO_INPUT_MONO8;                              // set_input_encoding
        int cov_mode = SVO_COV_OFF; double cov_sigma = 1.0;           // set_pose_covariance
        std::vector<uint8_t> mask;                                    // set_detection_mask with a size, packed; emptied once installed
        bool clahe_on = false; double clahe_clip = 2.0; int clahe_tx = 8, clahe_ty = 8;   // set_clahe
        int track_rows = 0;                                           // set_track_output; 0: off
        bool desc_on = false;                                         // set_descriptor_output, behind the track output
        int prior_mode = SVO_PRIOR_EXPLICIT;                          // set_motion_prior_mode
    };
    // svo_set_pose_covariance's and svo_set_clahe's checks of their arguments (svo_api.hip: check_cov_mode, check_clahe_params), for
    // the calls that come before there is a context to ask
    static void check_cov(int mode, double pixel_sigma) {
        if ((mode != SVO_COV_OFF && mode != SVO_COV_RESIDUAL && mode != SVO_COV_FIXED_SIGMA) ||
            (mode == SVO_COV_FIXED_SIGMA && !(pixel_sigma > 0 && std::isfinite(pixel_sigma))))
            throw std::runtime_error("set_pose_covariance: bad mode or pixel_sigma");
    }
    static void check_clahe(double clip, int tx, int ty) {
        if (tx < 1 || tx > 16 || ty < 1 || ty > 16 || !std::isfinite(clip)) throw std::runtime_error("set_clahe: tiles must be 1 .. 16 and clip finite");
    }
    // Every held setting onto ctx, a context just created for width x height frames, in the order both facades use: rectification,
    // projection, input format, covariance, detection mask, CLAHE (its fit check sees the raw size: after the rectification), track
    // output, descriptors (they ride on it), prior mode.
    void apply(svo_context* ctx, int width, int height) const {
        if (held_.rect) svo_throw(svo_set_rectification(ctx, -1, &held_.rect_l, &held_.rect_r));
        svo_throw(svo_set_projection(ctx, -1, leftCameraProjection_.data(), rightCameraProjection_.data()));
        if (held_.in_format != SVO_INPUT_MONO8) svo_throw(svo_set_input_format(ctx, held_.in_format));
        if (held_.cov_mode != SVO_COV_OFF) svo_throw(svo_set_pose_covariance(ctx, held_.cov_mode, held_.cov_sigma));
        if (!held_.mask.empty()) {
            if (held_.mask.size() != (size_t)width * height) throw std::runtime_error("set_detection_mask: the mask is not of the frame's size");
            svo_throw(svo_set_detection_mask(ctx, -1, held_.mask.data(), width, 0));
        }
        if (held_.clahe_on) svo_throw(svo_set_clahe(ctx, 1, held_.clahe_clip, held_.clahe_tx, held_.clahe_ty));
        if (held_.track_rows > 0) svo_throw(svo_set_track_output(ctx, 1, held_.track_rows));
        if (held_.track_rows > 0 && held_.desc_on) svo_throw(svo_set_descriptor_output(ctx, 1));
        if (held_.prior_mode != SVO_PRIOR_EXPLICIT) svo_throw(svo_set_motion_prior_mode(ctx, held_.prior_mode));
    }
    // The reference learns size and type from the first frame: create the context for it, apply what is held, and only then adopt it.
    // A setting the context refuses (CLAHE tiles that do not fit this size, ...) throws with the object still before its first frame
    // and everything held: correct the setting and pass the frame again.
    void first_frame(const Image& im) {
        cfg_.channels = held_.in_format != SVO_INPUT_MONO8 ? 1 : im.channels;   // an encoding's frames become mono8 inside ingest
        svo_context* ctx = nullptr;
        svo_throw(svo_create(&cfg_, default_device(), 1, im.cols, im.rows, &ctx));
        try { apply(ctx, im.cols, im.rows); } catch (...) { svo_destroy(ctx); throw; }
        ctx_ = ctx; width_ = im.cols; height_ = im.rows;
        held_.mask.clear(); held_.mask.shrink_to_fit();
    }
    svo_config cfg_;
    svo_context* ctx_ = nullptr;
    int width_ = 0, height_ = 0;                                      // learnt from the first frame
    Held held_;
};

// A device-resident index of (descriptor, id) rows with an exact 2-nearest-neighbour Hamming search (svo.h, "Descriptor index"): per
// query the best row of a range, and the best row with ANOTHER id.  add and match are synchronous and wait for the index's own stream
// only, so both may be called between a VisualOdometry's frames or while another context has frames in flight.
class DescriptorIndex {
   public:
    using Descriptor = std::array<uint8_t, SVO_DESC_BYTES>;
    explicit DescriptorIndex(int capacity, int device = default_device()) { svo_throw(svo_desc_index_create(device, capacity, &index_)); }
    ~DescriptorIndex() { svo_desc_index_destroy(index_); }
    DescriptorIndex(const DescriptorIndex&) = delete;
    DescriptorIndex& operator=(const DescriptorIndex&) = delete;
    DescriptorIndex(DescriptorIndex&& o) noexcept : index_(o.index_) { o.index_ = nullptr; }

    // append rows (all or none) -> the row number of the first one
    int add(const std::vector<Descriptor>& desc, const std::vector<uint64_t>& ids) {
        if (desc.size() != ids.size()) throw std::runtime_error("DescriptorIndex::add: one id per descriptor row expected");
        int first = 0;
        svo_throw(svo_desc_index_add(index_, (int)desc.size(), rows(desc), ids.data(), &first));
        return first;
    }
    // append the rows of vo's last stereo_callback whose flags contain need_flags (SVO_OBS_INLIER: its inliers) -> {first row, rows added}
    std::pair<int, int> add_frame(VisualOdometry& vo, uint32_t need_flags = SVO_OBS_INLIER) {
        int first = 0, n = 0;
        svo_throw(svo_desc_index_add_frame(index_, vo.need_frame("DescriptorIndex::add_frame"), 0, need_flags, &first, &n));
        return {first, n};
    }
    // per query the best and the second-best (by id) row of [row_lo, row_hi); row_hi = -1: every row from row_lo on
    std::vector<svo_desc_match> match(const std::vector<Descriptor>& query, int row_lo = 0, int row_hi = -1) {
        std::vector<svo_desc_match> out(query.size());
        svo_throw(svo_desc_index_match(index_, (int)query.size(), rows(query), row_lo, row_hi, out.data()));
        return out;
    }
    // ---- relocalisation (svo.h, "Relocalisation"): rows with 3-D points, and the camera's pose in the map from one call
    struct Candidates { std::vector<int32_t> query, row; std::vector<uint8_t> inlier; };   // inlier: localize only
    static svo_reloc_params default_params() { svo_reloc_params p; svo_reloc_params_default(&p); return p; }
    void enable_points() { svo_throw(svo_desc_index_enable_points(index_)); }              // while the index is empty
    // add with a point per row: xyz holds 3 floats per row in the map frame; tags (>= 0) may be empty: all 0
    int add_points(const std::vector<Descriptor>& desc, const std::vector<uint64_t>& ids, const std::vector<float>& xyz, const std::vector<int32_t>& tags = {}) {
        if (desc.size() != ids.size() || xyz.size() != 3 * desc.size() || (!tags.empty() && tags.size() != desc.size()))
            throw std::runtime_error("DescriptorIndex::add_points: one id, one point and one tag per descriptor row expected");
        int first = 0;
        svo_throw(svo_desc_index_add_points(index_, (int)desc.size(), rows(desc), ids.data(), xyz.data(),
                                            tags.empty() ? nullptr : tags.data(), &first));
        return first;
    }
    // add_frame with each row's point moved into the map.  cam_to_map: the pose (row-major 4 x 4) of the PREVIOUS frame's left camera
    // in the map — an observation row's xyz is in the T0 camera frame — or nullptr for the identity.
    std::pair<int, int> add_frame(VisualOdometry& vo, const double* cam_to_map, int32_t tag, uint32_t need_flags = SVO_OBS_INLIER) {
        int first = 0, n = 0;
        svo_throw(svo_desc_index_add_frame_points(index_, vo.need_frame("DescriptorIndex::add_frame"), 0, need_flags, cam_to_map, tag, &first, &n));
        return {first, n};
    }
    // the selection alone: the candidates' queries and rows, in increasing query
    Candidates select(const std::vector<Descriptor>& query, const std::vector<float>& xy, const svo_reloc_params& params) {
        return select_("select", nullptr, nullptr, query, xy, params);
    }
    // search, select and RANSAC-PnP: result.R, t hold the guess going in and the pose (x_cam = R X_map + t) on success, result.T the
    // camera in the map; candidates (may be null) receives the candidate lists with the PnP's inlier flags
    svo_reloc_result localize(const float K[9], const std::vector<Descriptor>& query, const std::vector<float>& xy, const svo_reloc_params& params,
                              svo_reloc_result result, Candidates* candidates = nullptr) {
        return localize_("localize", K, nullptr, query, xy, params, result, candidates);
    }
    // ---- guided search (svo.h, "Guided search"): the same calls over the rows a pose prior projects near each query's pixel
    // a guide from the prior x_cam = R X_map + t (row-major 3 x 3, 3) and the gate's radius in pixels
    static svo_reloc_guide guide(const double R[9], const double t[3], float radius) {
        svo_reloc_guide g;
        for (int i = 0; i < 9; i++) g.R[i] = R[i];
        for (int i = 0; i < 3; i++) g.t[i] = t[i];
        g.radius = radius; g.reserved = 0;
        return g;
    }
    // the projections of rows [row_lo, row_hi) with the prior, 2 floats per row; an invisible row is (+inf, +inf)
    std::vector<float> project(const float K[9], const svo_reloc_guide& g, int row_lo = 0, int row_hi = -1) {
        const int hi = row_hi == -1 ? size() : row_hi;
        std::vector<float> uv(2 * (size_t)(hi > row_lo ? hi - row_lo : 0));
        svo_throw(svo_desc_index_project(index_, K, &g, row_lo, row_hi, uv.data()));
        return uv;
    }
    std::vector<svo_desc_match> match_guided(const float K[9], const svo_reloc_guide& g, const std::vector<Descriptor>& query, const std::vector<float>& xy,
                                             int row_lo = 0, int row_hi = -1) {
        one_pixel_each("match_guided", query, xy);
        std::vector<svo_desc_match> out(query.size());
        svo_throw(svo_desc_index_match_guided(index_, K, &g, (int)query.size(), rows(query), xy.data(), row_lo, row_hi, out.data()));
        return out;
    }
    Candidates select_guided(const float K[9], const svo_reloc_guide& g, const std::vector<Descriptor>& query, const std::vector<float>& xy,
                             const svo_reloc_params& params) {
        return select_("select_guided", K, &g, query, xy, params);
    }
    // result.R, t: the PnP's guess going in — the guide's R, t is the usual choice
    svo_reloc_result localize_guided(const float K[9], const svo_reloc_guide& g, const std::vector<Descriptor>& query, const std::vector<float>& xy,
                                     const svo_reloc_params& params, svo_reloc_result result, Candidates* candidates = nullptr) {
        return localize_("localize_guided", K, &g, query, xy, params, result, candidates);
    }
    void set_guided_sort(bool on) { svo_throw(svo_desc_index_set_guided_sort(index_, on ? 1 : 0)); }
    // ---- batched relocalisation (svo.h, "Batched relocalisation"): many cameras in one call
    // One camera of a batch.  In: K, the guide (read by a guided batch only), the queries with a pixel each, and result.R, t, the
    // PnP's guess.  Out: result and candidates, what localize / localize_guided return for this camera alone, bit for bit.
    struct BatchCamera {
        float K[9];
        svo_reloc_guide guide;
        std::vector<Descriptor> query;
        std::vector<float> xy;
        svo_reloc_result result;
        Candidates candidates;
    };
    // localize_guided (guided) or localize for the n_cameras cameras at cams, in one call and one synchronisation
    void localize_batch(BatchCamera* cams, size_t n_cameras, bool guided, const svo_reloc_params& params) {
        std::vector<float> K(9 * n_cameras), xy;
        std::vector<svo_reloc_guide> guides(guided ? n_cameras : 0);
        std::vector<int32_t> begin(n_cameras + 1, 0);
        std::vector<Descriptor> query;
        std::vector<svo_reloc_result> results(n_cameras);
        for (size_t b = 0; b < n_cameras; b++) {
            one_pixel_each("localize_batch", cams[b].query, cams[b].xy);
            for (int i = 0; i < 9; i++) K[9 * b + (size_t)i] = cams[b].K[i];
            if (guided) guides[b] = cams[b].guide;
            query.insert(query.end(), cams[b].query.begin(), cams[b].query.end());
            xy.insert(xy.end(), cams[b].xy.begin(), cams[b].xy.end());
            begin[b + 1] = (int32_t)query.size();
            results[b] = cams[b].result;
        }
        Candidates all = room(query.size(), true);
        svo_throw(svo_desc_index_localize_batch(index_, (int)n_cameras, K.data(), guided ? guides.data() : nullptr, begin.data(), rows(query), xy.data(), &params,
                                                results.data(), all.query.data(), all.row.data(), all.inlier.data()));
        for (size_t b = 0; b < n_cameras; b++) {
            const size_t lo = (size_t)begin[b], k = (size_t)results[b].n_candidates;
            cams[b].result = results[b];
            cams[b].candidates.query.assign(all.query.begin() + (long)lo, all.query.begin() + (long)(lo + k));
            cams[b].candidates.row.assign(all.row.begin() + (long)lo, all.row.begin() + (long)(lo + k));
            cams[b].candidates.inlier.assign(all.inlier.begin() + (long)lo, all.inlier.begin() + (long)(lo + k));
        }
    }
    // diagnostics: the lane order of the last localize_batch as global query numbers
    std::vector<int32_t> batch_order() {
        int n = 0;
        svo_throw(svo_desc_index_get_batch_order(index_, 0, nullptr, &n));
        std::vector<int32_t> order((size_t)n);
        svo_throw(svo_desc_index_get_batch_order(index_, n, order.data(), &n));
        return order;
    }
    // ---- index maintenance (svo.h, "Index maintenance"): drop rows anywhere and move points, both on the device
    // a rule over the scope [row_lo, row_hi) with no flag set: set flags, the tag window and the id list (which must outlive the call)
    static svo_retire_rule retire_rule(int row_lo = 0, int row_hi = -1) {
        svo_retire_rule r;
        r.flags = 0; r.row_lo = row_lo; r.row_hi = row_hi; r.tag_lo = 0; r.tag_hi = 0; r.n_ids = 0; r.ids = nullptr;
        return r;
    }
    // drop what the rule says and close the gaps in place -> kept_before, size-before + 1 entries: row r became row kept_before[r],
    // and the last entry is the new size
    std::vector<int32_t> retire(const svo_retire_rule& rule) {
        std::vector<int32_t> kept_before((size_t)size() + 1);
        svo_throw(svo_desc_index_retire(index_, &rule, kept_before.data(), nullptr));
        return kept_before;
    }
    // the points of rows [rows.first, rows.second) whose tag lies in [tags.first, tags.second] through T (row-major 4 x 4)
    // -> {moved, skipped}: a skipped row's result was not finite in float and the row is unchanged
    std::pair<int, int> transform_points(const double T[16], std::pair<int, int> rows = {0, -1}, std::pair<int32_t, int32_t> tags = {0, INT32_MAX}) {
        int moved = 0, skipped = 0;
        svo_throw(svo_desc_index_transform_points(index_, T, rows.first, rows.second, tags.first, tags.second, &moved, &skipped));
        return {moved, skipped};
    }
    // ---- map alignment (svo.h, "Map alignment"): the rigid transform between two row spans, found on the device
    struct Pairs { std::vector<int32_t> src, dst; std::vector<uint8_t> inlier; };          // inlier: align only
    // svo_align_params_default; the caller sets the spans.  inlier_dist has no default: none has been measured for any rig
    static svo_align_params align_params(float inlier_dist) { svo_align_params p; svo_align_params_default(&p, inlier_dist); return p; }
    // match with the descriptors of rows [src.first, src.second) as the queries, over rows [dst.first, dst.second)
    std::vector<svo_desc_match> match_rows(std::pair<int, int> src, std::pair<int, int> dst) {
        std::vector<svo_desc_match> out(span_rows(src.first, src.second));
        svo_throw(svo_desc_index_match_rows(index_, src.first, src.second, dst.first, dst.second, out.data()));
        return out;
    }
    // rules 1 - 5: one pair of rows per landmark on either side, in increasing source row
    Pairs pair_rows(const svo_align_params& prm) {
        Pairs p = pairs_room(prm, false);
        int k = 0;
        svo_throw(svo_desc_index_pair_rows(index_, &prm, &k, p.src.data(), p.dst.data()));
        p.src.resize((size_t)k); p.dst.resize((size_t)k);
        return p;
    }
    // x_dst = R x_src + t between the source span's landmarks and their matches; result.T is transform_points' argument
    svo_align_result align(const svo_align_params& prm, Pairs* pairs = nullptr) {
        Pairs p = pairs_room(prm, true);
        svo_align_result r;
        svo_throw(svo_desc_index_align(index_, &prm, &r, p.src.data(), p.dst.data(), p.inlier.data()));
        p.src.resize((size_t)r.n_pairs); p.dst.resize((size_t)r.n_pairs); p.inlier.resize((size_t)r.n_pairs);
        if (pairs) *pairs = std::move(p);
        return r;
    }
    // ---- landmark fusion (svo.h, "Landmark fusion"): one id per landmark where two spans of rows overlap, on the device
    // svo_fuse_params_default; the caller sets the spans.  radius (the map's unit) has no default: none has been measured for any rig
    static svo_fuse_params fuse_params(float radius) { svo_fuse_params p; svo_fuse_params_default(&p, radius); return p; }
    // match_rows among the rows of dst whose point lies within radius of the source row's on every axis
    std::vector<svo_desc_match> match_near(std::pair<int, int> src, std::pair<int, int> dst, float radius) {
        std::vector<svo_desc_match> out(span_rows(src.first, src.second));
        svo_throw(svo_desc_index_match_near(index_, src.first, src.second, dst.first, dst.second, radius, out.data()));
        return out;
    }
    // rules 1 - 3, the dry run of fuse: one pair of rows per landmark on either side, in increasing source row
    Pairs pair_near(const svo_fuse_params& prm) {
        const size_t n = span_rows(prm.src_lo, prm.src_hi);
        Pairs p; p.src.resize(n); p.dst.resize(n);
        int k = 0;
        svo_throw(svo_desc_index_pair_near(index_, &prm, &k, p.src.data(), p.dst.data()));
        p.src.resize((size_t)k); p.dst.resize((size_t)k);
        return p;
    }
    // every row of [rows.first, rows.second) whose id is from_ids[i] gets to_ids[i], in one simultaneous step -> the rows changed
    int relabel(const std::vector<uint64_t>& from_ids, const std::vector<uint64_t>& to_ids, std::pair<int, int> rows = {0, -1}) {
        if (from_ids.size() != to_ids.size()) throw std::runtime_error("DescriptorIndex::relabel: one `to` id per `from` id expected");
        if (from_ids.size() > (size_t)SVO_FUSE_MAX_LIST) throw std::runtime_error("DescriptorIndex::relabel: at most 1 << 20 entries");
        int changed = 0;
        svo_throw(svo_desc_index_relabel(index_, (int)from_ids.size(), from_ids.data(), to_ids.data(), rows.first, rows.second, &changed));
        return changed;
    }
    // the source span's landmarks take the ids of their partners in the destination span, in the rows of the relabel span
    svo_fuse_result fuse(const svo_fuse_params& prm, Pairs* pairs = nullptr) {
        const size_t n = span_rows(prm.src_lo, prm.src_hi);
        Pairs p; p.src.resize(n); p.dst.resize(n);
        svo_fuse_result r;
        svo_throw(svo_desc_index_fuse(index_, &prm, &r, p.src.data(), p.dst.data()));
        p.src.resize((size_t)r.n_pairs); p.dst.resize((size_t)r.n_pairs);
        if (pairs) *pairs = std::move(p);
        return r;
    }
    // ---- place candidates (svo.h, "Place candidates"): which keyframes (tags) of the map a frame resembles, on the device
    static svo_place_params place_params() { svo_place_params p; svo_place_params_default(&p); return p; }
    struct Places { svo_place_result result; std::vector<svo_place> places; };              // places: rule 3's order
    struct TagVotes { std::vector<int32_t> votes, rows, row_first, row_end; };               // indexed tag - tags.first
    // rules 1 - 3: the keyframes whose rows hold the most landmarks these descriptors recognise; cand: the recognised landmarks, as select's
    Places places(const std::vector<Descriptor>& query, const svo_place_params& prm, Candidates* cand = nullptr) {
        if (query.size() > (size_t)SVO_PLACE_MAX_IDS) throw std::runtime_error("DescriptorIndex::places: at most 4096 queries");
        Places p; p.places.resize(SVO_PLACE_MAX_PLACES);
        Candidates c = room(query.size(), false);
        svo_throw(svo_desc_index_places(index_, (int)query.size(), rows(query), &prm, &p.result, p.places.data(), c.query.data(), c.row.data()));
        p.places.resize((size_t)p.result.n_places);
        shrink(c, query.empty() ? 0 : p.result.n_landmarks);
        if (cand) *cand = std::move(c);
        return p;
    }
    // rules 2 - 3 for landmarks known by id: the keyframes that saw what a tracker holds
    Places places_from_ids(const std::vector<uint64_t>& ids, const svo_place_params& prm) {
        if (ids.size() > (size_t)SVO_PLACE_MAX_IDS) throw std::runtime_error("DescriptorIndex::places_from_ids: at most 4096 ids");
        Places p; p.places.resize(SVO_PLACE_MAX_PLACES);
        svo_throw(svo_desc_index_places_from_ids(index_, (int)ids.size(), ids.data(), &prm, &p.result, p.places.data()));
        p.places.resize((size_t)p.result.n_places);
        return p;
    }
    // rule 2 alone: per tag of [tags.first, tags.second] the rows of [rows.first, rows.second) under it and those whose id is listed
    TagVotes tag_votes(const std::vector<uint64_t>& ids, std::pair<int, int> rows = {0, -1}, std::pair<int32_t, int32_t> tags = {0, 0}) {
        if (ids.size() > (size_t)SVO_PLACE_MAX_IDS) throw std::runtime_error("DescriptorIndex::tag_votes: at most 4096 ids");
        const int64_t span = (int64_t)tags.second - (int64_t)tags.first + 1;
        const size_t nb = tags.first >= 0 && span >= 1 && span <= SVO_PLACE_MAX_TAGS ? (size_t)span : 1;   // a span the library refuses: room for nothing
        TagVotes v; v.votes.resize(nb); v.rows.resize(nb); v.row_first.resize(nb); v.row_end.resize(nb);
        svo_throw(svo_desc_index_tag_votes(index_, (int)ids.size(), ids.data(), rows.first, rows.second, tags.first, tags.second, v.votes.data(),
                                           v.rows.data(), v.row_first.data(), v.row_end.data()));
        return v;
    }
    // ---- batched place candidates (svo.h, "Batched place candidates"): every camera's keyframe votes in one call
    // camera b's result is what the single call returns for ids[b] or query[b] alone, bit for bit
    struct TagVotesBatch { std::vector<int32_t> votes, rows, row_first, row_end; size_t n_bins; };   // votes: camera-major, votes[b * n_bins + tag - tags.first]
    std::vector<Places> places_from_ids_batch(const std::vector<std::vector<uint64_t>>& ids, const svo_place_params& prm) {
        std::vector<int32_t> begin;
        const std::vector<uint64_t> all = concat_(ids, begin);
        PlacesRoom r(ids.size(), prm);
        svo_throw(svo_desc_index_places_from_ids_batch(index_, (int)ids.size(), begin.data(), all.data(), &prm, r.results.data(), r.places.data()));
        return r.split();
    }
    // cands: per camera the recognised landmarks, query numbers inside the camera's own vector
    std::vector<Places> places_batch(const std::vector<std::vector<Descriptor>>& query, const svo_place_params& prm, std::vector<Candidates>* cands = nullptr) {
        std::vector<int32_t> begin;
        const std::vector<Descriptor> all = concat_(query, begin);
        PlacesRoom r(query.size(), prm);
        Candidates c = room(all.size(), false);
        svo_throw(svo_desc_index_places_batch(index_, (int)query.size(), begin.data(), rows(all), &prm, r.results.data(), r.places.data(), c.query.data(),
                                              c.row.data()));
        if (cands) {
            cands->assign(query.size(), Candidates());
            for (size_t b = 0; b < query.size(); b++) {
                const long lo = (long)begin[b], k = query[b].empty() ? 0 : (long)r.results[b].n_landmarks;
                (*cands)[b].query.assign(c.query.begin() + lo, c.query.begin() + lo + k);
                (*cands)[b].row.assign(c.row.begin() + lo, c.row.begin() + lo + k);
            }
        }
        return r.split();
    }
    TagVotesBatch tag_votes_batch(const std::vector<std::vector<uint64_t>>& ids, std::pair<int, int> rows = {0, -1}, std::pair<int32_t, int32_t> tags = {0, 0}) {
        std::vector<int32_t> begin;
        const std::vector<uint64_t> all = concat_(ids, begin);
        const int64_t span = (int64_t)tags.second - (int64_t)tags.first + 1;
        const bool fits = tags.first >= 0 && span >= 1 && span <= SVO_PLACE_MAX_TAGS && (int64_t)ids.size() * span <= SVO_PLACE_BATCH_MAX_BINS;
        TagVotesBatch v; v.n_bins = fits ? (size_t)span : 1;   // a span the library refuses: room for nothing
        v.votes.resize(fits ? ids.size() * v.n_bins : 1); v.rows.resize(v.n_bins); v.row_first.resize(v.n_bins); v.row_end.resize(v.n_bins);
        svo_throw(svo_desc_index_tag_votes_batch(index_, (int)ids.size(), begin.data(), all.data(), rows.first, rows.second, tags.first, tags.second,
                                                 v.votes.data(), v.rows.data(), v.row_first.data(), v.row_end.data()));
        return v;
    }
    // ---- landmark consolidation (svo.h, "Landmark consolidation"): one row per landmark, and the rows read back
    // svo_consolidate_params_default: the whole index, every tag.  radius (the map's unit) has no default: none has been measured
    static svo_consolidate_params consolidate_params(float radius) { svo_consolidate_params p; svo_consolidate_params_default(&p, radius); return p; }
    // each group's latest row takes the medoid descriptor and the gated mean point, the others go; kept_before: retire's remapping
    svo_consolidate_result consolidate(const svo_consolidate_params& prm, std::vector<int32_t>* kept_before = nullptr) {
        std::vector<int32_t> map((size_t)size() + 1);
        svo_consolidate_result r;
        svo_throw(svo_desc_index_consolidate(index_, &prm, &r, map.data()));
        if (kept_before) *kept_before = std::move(map);
        return r;
    }
    struct Rows { std::vector<Descriptor> desc; std::vector<uint64_t> ids; std::vector<float> xyz; std::vector<int32_t> tags; };
    // rows [row_lo, row_hi) back on the host; xyz (3 floats a row, +inf without a point) and tags only on an index with points
    Rows read_rows(int row_lo = 0, int row_hi = -1, bool points = true) {
        const size_t n = span_rows(row_lo, row_hi);
        Rows r; r.desc.resize(n); r.ids.resize(n); r.xyz.resize(points ? 3 * n : 0); r.tags.resize(points ? n : 0);
        svo_throw(svo_desc_index_read_rows(index_, row_lo, row_hi, n ? r.desc[0].data() : nullptr, r.ids.data(), points ? r.xyz.data() : nullptr,
                                           points ? r.tags.data() : nullptr));
        return r;
    }
    // ---- batched insertion (svo.h, "Batched insertion"): many sequences of a context's last collected frame, or the caller's own
    // observation rows, filtered, packed and transformed on the device in one call
    struct Inserted { std::vector<int32_t> first_row, n_added; };
    // what a call may give per entry; an empty vector is the C call's NULL (every sequence in order, no id offset, xyz as it is, tag 0)
    struct InsertArgs {
        std::vector<int32_t> seqs;                 // add_frames only
        std::vector<uint64_t> id_base;
        std::vector<double> cam_to_map;            // 16 per entry, with points only
        std::vector<int32_t> tags;                 // with points only
    };
    // n: the entries (with seqs given, seqs.size()).  with_points: svo_desc_index_add_frames_points
    Inserted add_frames(svo_context* ctx, int n, bool with_points = false, const InsertArgs& a = InsertArgs(), uint32_t need_flags = SVO_OBS_INLIER) {
        if (!a.seqs.empty()) n = (int)a.seqs.size();
        insert_sizes("add_frames", n, a);
        Inserted r; r.first_row.resize((size_t)(n > 0 ? n : 0)); r.n_added.resize(r.first_row.size());
        if (with_points)
            svo_throw(svo_desc_index_add_frames_points(index_, ctx, n, opt(a.seqs), need_flags, opt(a.id_base), opt(a.cam_to_map), opt(a.tags), r.first_row.data(), r.n_added.data()));
        else
            svo_throw(svo_desc_index_add_frames(index_, ctx, n, opt(a.seqs), need_flags, opt(a.id_base), r.first_row.data(), r.n_added.data()));
        return r;
    }
    // entry b: the rows [row_begin[b], row_begin[b + 1]) of obs and desc
    Inserted add_obs(const std::vector<int32_t>& row_begin, const std::vector<svo_track_obs>& obs, const std::vector<Descriptor>& desc, bool with_points = false,
                     const InsertArgs& a = InsertArgs(), uint32_t need_flags = SVO_OBS_INLIER) {
        const int n = row_begin.empty() ? 0 : (int)row_begin.size() - 1;
        if (obs.size() != desc.size() || (n > 0 && (size_t)row_begin.back() != obs.size())) throw std::runtime_error("DescriptorIndex::add_obs: one descriptor per observation row, row_begin ending at their number, expected");
        insert_sizes("add_obs", n, a);
        Inserted r; r.first_row.resize((size_t)n); r.n_added.resize((size_t)n);
        svo_throw(svo_desc_index_add_obs(index_, n, row_begin.data(), obs.data(), rows(desc), need_flags, opt(a.id_base), with_points ? 1 : 0, opt(a.cam_to_map), opt(a.tags),
                                         r.first_row.data(), r.n_added.data()));
        return r;
    }
    svo_desc_insert_stats insert_stats() const { svo_desc_insert_stats s; svo_throw(svo_desc_index_get_insert_stats(index_, &s)); return s; }
    int retire_slab_rows() const { return svo_desc_index_get_retire_slab_rows(index_); }
    void retire_slab_rows(int rows) { svo_throw(svo_desc_index_set_retire_slab_rows(index_, rows)); }   // 0: the default
    int size() const { return svo_desc_index_size(index_); }
    void truncate(int n_rows) { svo_throw(svo_desc_index_truncate(index_, n_rows)); }
    svo_desc_index* handle() { return index_; }

   private:
    // the rows of a possibly empty descriptor vector
    static const uint8_t* rows(const std::vector<Descriptor>& d) { return d.empty() ? nullptr : d[0].data(); }
    // an optional per-entry array of a batched insertion, and their sizes against the entries
    template <typename T> static const T* opt(const std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }
    static void insert_sizes(const char* what, int n, const InsertArgs& a) {
        const size_t m = (size_t)(n > 0 ? n : 0);
        if ((!a.id_base.empty() && a.id_base.size() != m) || (!a.cam_to_map.empty() && a.cam_to_map.size() != 16 * m) || (!a.tags.empty() && a.tags.size() != m))
            throw std::runtime_error(std::string("DescriptorIndex::") + what + ": id_base, cam_to_map (16 each) and tags hold one per entry, or nothing");
    }
    // the rows of a span as the library will resolve it (0 for one it will refuse), and the room for its pairs
    size_t span_rows(int lo, int hi) const { const int h = hi == -1 || hi > size() ? size() : hi; return lo >= 0 && h > lo ? (size_t)(h - lo) : 0; }
    Pairs pairs_room(const svo_align_params& prm, bool inlier) const {
        const size_t n = span_rows(prm.src_lo, prm.src_hi);
        Pairs p; p.src.resize(n); p.dst.resize(n); p.inlier.resize(inlier ? n : 0);
        return p;
    }
    static void one_pixel_each(const char* what, const std::vector<Descriptor>& query, const std::vector<float>& xy) {
        if (xy.size() != 2 * query.size()) throw std::runtime_error(std::string("DescriptorIndex::") + what + ": one pixel per query expected");
    }
    // the candidate lists of a call over n queries, with or without the inlier list: sized before the call, cut to its count after
    static Candidates room(size_t n, bool inlier) { Candidates c; c.query.resize(n); c.row.resize(n); c.inlier.resize(inlier ? n : 0); return c; }
    static void shrink(Candidates& c, int k) { c.query.resize((size_t)k); c.row.resize((size_t)k); if (!c.inlier.empty()) c.inlier.resize((size_t)k); }
    // a batch's per-camera vectors as one, with the n + 1 offsets the C call takes
    template <typename T> static std::vector<T> concat_(const std::vector<std::vector<T>>& per_camera, std::vector<int32_t>& begin) {
        std::vector<T> all;
        begin.assign(1, 0);
        for (const std::vector<T>& v : per_camera) {
            all.insert(all.end(), v.begin(), v.end());
            begin.push_back((int32_t)all.size());
        }
        return all;
    }
    // the results of a batched places call: sized before the call, split per camera after
    struct PlacesRoom {
        std::vector<svo_place_result> results;
        std::vector<svo_place> places;
        size_t per_camera;
        PlacesRoom(size_t n_cameras, const svo_place_params& prm)
            : results(n_cameras), per_camera(prm.max_places >= 1 && prm.max_places <= SVO_PLACE_MAX_PLACES ? (size_t)prm.max_places : 1) {
            places.resize(n_cameras * per_camera);
        }
        std::vector<Places> split() const {
            std::vector<Places> out(results.size());
            for (size_t b = 0; b < results.size(); b++) {
                out[b].result = results[b];
                out[b].places.assign(places.begin() + (long)(b * per_camera), places.begin() + (long)(b * per_camera) + results[b].n_places);
            }
            return out;
        }
    };
    // select and localize; g (with its K) null: the unguided search
    Candidates select_(const char* what, const float* K, const svo_reloc_guide* g, const std::vector<Descriptor>& query, const std::vector<float>& xy,
                       const svo_reloc_params& params) {
        one_pixel_each(what, query, xy);
        Candidates c = room(query.size(), false);
        int k = 0, n = (int)query.size();
        svo_throw(g ? svo_desc_index_select_guided(index_, K, g, n, rows(query), xy.data(), &params, &k, c.query.data(), c.row.data(), nullptr, nullptr)
                    : svo_desc_index_select(index_, n, rows(query), xy.data(), &params, &k, c.query.data(), c.row.data(), nullptr, nullptr));
        shrink(c, k);
        return c;
    }
    svo_reloc_result localize_(const char* what, const float* K, const svo_reloc_guide* g, const std::vector<Descriptor>& query, const std::vector<float>& xy,
                               const svo_reloc_params& params, svo_reloc_result result, Candidates* candidates) {
        one_pixel_each(what, query, xy);
        Candidates c = room(query.size(), true);
        const int n = (int)query.size();
        svo_throw(g ? svo_desc_index_localize_guided(index_, K, g, n, rows(query), xy.data(), &params, &result, c.query.data(), c.row.data(), c.inlier.data())
                    : svo_desc_index_localize(index_, K, n, rows(query), xy.data(), &params, &result, c.query.data(), c.row.data(), c.inlier.data()));
        shrink(c, result.n_candidates);
        if (candidates) *candidates = std::move(c);
        return result;
    }
    svo_desc_index* index_ = nullptr;
};

}   // namespace visual_odometry
