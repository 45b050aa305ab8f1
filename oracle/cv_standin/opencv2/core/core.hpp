// ============================================================================
// TEST INFRASTRUCTURE ONLY.  This project's own stand-in for the OpenCV
// headers that the reference's DBoW2 and its ORB extractor include, written
// from scratch.  It exists so that oracle/dbow2_ref.cpp and oracle/orb_ref.cpp
// can compile the reference's code where it lies; nothing of the product
// includes it.  Every other header under cv_standin/ forwards to this one.
//   cv::Mat          row-major bytes or floats; owns its store (shared on
//                    copy, compact and deep on clone()) or is a view: a row /
//                    column range or Rect of another Mat, or caller memory
//                    with a given step
//   cv::Point_<T>, Size, Rect, KeyPoint: plain data
//   cvRound (half to even), cvFloor, cvCeil, CV_PI
//   cv::fastAtan2    DECLARED here, defined in cv_standin/fast_atan2.cpp (the
//                    rule of include/gmmloc_hip.h, one IEEE operation per
//                    step; that file is always compiled -ffp-contract=off)
//   cv::FAST, resize, GaussianBlur: DECLARED here, defined in
//                    cv_standin/hooks.cpp: each calls through a function
//                    pointer whose default throws "not provided" - OpenCV's
//                    FAST, resize and blur are nobody's to pin here; a wrapper
//                    sets the pointers so that the reference's code AROUND
//                    them runs (oracle/orb_detect_ref.cpp)
//   cv::copyMakeBorder  BORDER_REFLECT_101, in cv_standin/hooks.cpp
//   cv::KeyPointsFilter present so that ComputeKeyPointsOld compiles; throws
//   cv::FileStorage  present so that the YAML save / load members compile:
//   cv::FileNode     never open, every use throws
// The standard headers at the end of the list are the ones the reference's
// sources expect to arrive with OpenCV's (pow, log, memcpy, stringstream, sort).
// ============================================================================
#ifndef GMMLOC_ORACLE_CV_STANDIN_CORE_HPP
#define GMMLOC_ORACLE_CV_STANDIN_CORE_HPP

#include <cstddef>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <assert.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <iostream>
#include <sstream>

#define CV_8U 0
#define CV_32F 5
#define CV_8UC1 CV_8U
#define CV_PI 3.1415926535897932384626433832795

typedef unsigned char uchar;

// round to nearest, half to even (the default rounding mode is never changed here)
inline int cvRound(double v) { return (int)lrint(v); }
inline int cvRound(float v) { return (int)lrintf(v); }
inline int cvRound(int v) { return v; }
inline int cvFloor(double v) { return (int)floor(v); }
inline int cvFloor(float v) { return (int)floorf(v); }
inline int cvCeil(double v) { return (int)ceil(v); }
inline int cvCeil(float v) { return (int)ceilf(v); }

namespace cv {

template <class T>
class Point_ {
 public:
  T x, y;
  Point_() : x(0), y(0) {}
  Point_(T x_, T y_) : x(x_), y(y_) {}
  template <class S>
  Point_& operator*=(S s) {
    x = (T)(x * s);
    y = (T)(y * s);
    return *this;
  }
};
typedef Point_<int> Point2i;
typedef Point_<float> Point2f;
typedef Point2i Point;

class Size {
 public:
  int width, height;
  Size() : width(0), height(0) {}
  Size(int w, int h) : width(w), height(h) {}
};

class Rect {
 public:
  int x, y, width, height;
  Rect() : x(0), y(0), width(0), height(0) {}
  Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};

class KeyPoint {
 public:
  Point2f pt;
  float size = 0.f, angle = -1.f, response = 0.f;
  int octave = 0, class_id = -1;
  KeyPoint() {}
  KeyPoint(float x, float y, float size_, float angle_ = -1.f, float response_ = 0.f, int octave_ = 0, int class_id_ = -1)
      : pt(x, y), size(size_), angle(angle_), response(response_), octave(octave_), class_id(class_id_) {}
};

class Mat {
 public:
  int rows = 0, cols = 0;
  unsigned char* data = nullptr;
  size_t step = 0;  // bytes from one row to the next

  Mat() {}
  Mat(int r, int c, int type) { create(r, c, type); }
  Mat(Size s, int type) { create(s.height, s.width, type); }
  // a view of caller memory: nothing is copied or freed
  Mat(int r, int c, int type, void* caller, size_t step_) : rows(r), cols(c), data((unsigned char*)caller), step(step_), type_(type) {
    if (step < (size_t)c * elem_size(type)) throw std::runtime_error("cv stand-in: step below a row's bytes");
  }

  void create(int r, int c, int type) {
    if (data && r == rows && c == cols && type == type_) return;
    const size_t row = (size_t)c * elem_size(type);
    store_ = std::make_shared<std::vector<unsigned char>>((size_t)r * row);
    rows = r, cols = c, type_ = type, step = row;
    data = store_->data();
  }
  void create(Size s, int type) { create(s.height, s.width, type); }
  // Mat::zeros is an EXPRESSION as in OpenCV: assigned to a matrix that already has its size and type it is written INTO that matrix
  // (create() leaves it as it lies), so a row range of a larger matrix stays a view of it - ORBextractor::detect relies on that
  // (:1033-1034, :981).  Elsewhere it makes a new store.
  struct Zeros {
    int rows, cols, type;
  };
  static Zeros zeros(int r, int c, int type) { return Zeros{r, c, type}; }
  static Zeros zeros(Size s, int type) { return Zeros{s.height, s.width, type}; }
  Mat(const Zeros& z) { *this = z; }
  Mat& operator=(const Zeros& z) {
    create(z.rows, z.cols, z.type);
    for (int r = 0; r < rows; ++r) std::memset(data + (size_t)r * step, 0, (size_t)cols * elem_size(type_));
    return *this;
  }
  // where this matrix lies in the store it shares (a wrapper reports a view's offset with these); caller memory has no store
  const unsigned char* standin_store_begin() const { return store_ ? store_->data() : nullptr; }
  size_t standin_store_size() const { return store_ ? store_->size() : 0; }
  Mat clone() const {  // compact, whatever the step of this one
    Mat m;
    if (data) {
      m.create(rows, cols, type_);
      for (int r = 0; r < rows; ++r) std::memcpy(m.data + (size_t)r * m.step, data + (size_t)r * step, m.step);
    }
    return m;
  }
  void release() {
    store_.reset();
    rows = cols = 0;
    step = 0;
    data = nullptr;
  }
  bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
  int type() const { return type_; }
  size_t elemSize() const { return elem_size(type_); }
  size_t step1() const { return step / elem_size(type_); }

  unsigned char* ptr(int row = 0) { return data + (size_t)row * step; }
  const unsigned char* ptr(int row = 0) const { return data + (size_t)row * step; }
  template <class T>
  T* ptr(int row = 0) {
    return reinterpret_cast<T*>(data + (size_t)row * step);
  }
  template <class T>
  const T* ptr(int row = 0) const {
    return reinterpret_cast<const T*>(data + (size_t)row * step);
  }
  template <class T>
  T& at(int row, int col) {
    return reinterpret_cast<T*>(data + (size_t)row * step)[col];
  }
  template <class T>
  const T& at(int row, int col) const {
    return reinterpret_cast<const T*>(data + (size_t)row * step)[col];
  }

  // views: rows [r0, r1), columns [c0, c1); they share the store of this one
  Mat rowRange(int r0, int r1) const { return view(r0, r1, 0, cols); }
  Mat colRange(int c0, int c1) const { return view(0, rows, c0, c1); }
  Mat operator()(const Rect& r) const { return view(r.y, r.y + r.height, r.x, r.x + r.width); }

 private:
  static size_t elem_size(int type) {
    if (type == CV_8U) return 1;
    if (type == CV_32F) return 4;
    throw std::runtime_error("cv stand-in: element type not provided");
  }
  Mat view(int r0, int r1, int c0, int c1) const {
    if (r0 < 0 || r1 < r0 || r1 > rows || c0 < 0 || c1 < c0 || c1 > cols) throw std::runtime_error("cv stand-in: range outside the matrix");
    Mat m(*this);
    m.rows = r1 - r0, m.cols = c1 - c0;
    m.data = data + (size_t)r0 * step + (size_t)c0 * elem_size(type_);
    return m;
  }
  std::shared_ptr<std::vector<unsigned char>> store_;
  int type_ = CV_8U;
};

// include/gmmloc_hip.h's `angle` row -> degrees in [0, 360].  The stand-in also keeps the arguments of the calling thread's last call,
// so that a wrapper can read back the moments that the reference hands over and never returns.
float fastAtan2(float y, float x);
void standin_last_atan2_args(float* y, float* x);

enum { BORDER_REFLECT_101 = 4, BORDER_ISOLATED = 16 };
enum { INTER_LINEAR = 1 };

inline void standin_not_provided(const char* what) { throw std::runtime_error(std::string("cv stand-in: ") + what + " is not provided"); }
// DECLARED here, defined in cv_standin/hooks.cpp.  FAST, resize and GaussianBlur call through the pointers below, whose default throws
// "not provided": a wrapper that wants the extractor's detection half to run sets them.  The destination is an output array as OpenCV
// has it: created at the size asked for, which leaves a destination of that size - a view into a larger matrix included - as it lies.
// This stand-in takes it by value, so a destination of ANOTHER size cannot be handed back and throws.
//   FAST            hook(image view, key-points, threshold, nonmax): the view's data / step tell where in its parent it lies
//   resize          hook(src, dst): dst has the size asked for; INTER_LINEAR only
//   GaussianBlur    hook(src, dst, ksize, sigma): src is a compact copy, so the call may be in place; square kernels only
//   copyMakeBorder  implemented: BORDER_REFLECT_101, with or without BORDER_ISOLATED (the source is never read beyond its own range,
//                   which is what OpenCV does for a matrix that is no view and for an ISOLATED view).  A destination that already
//                   holds the source as its view at (top, left) keeps those bytes; only the border is written.
typedef void (*standin_fast_fn)(const Mat& image, std::vector<KeyPoint>& keypoints, int threshold, bool nonmax);
typedef void (*standin_resize_fn)(const Mat& src, Mat& dst);
typedef void (*standin_blur_fn)(const Mat& src, Mat& dst, int ksize, double sigma);
extern standin_fast_fn standin_fast;
extern standin_resize_fn standin_resize;
extern standin_blur_fn standin_blur;
void FAST(const Mat& image, std::vector<KeyPoint>& keypoints, int threshold, bool nonmax = true);
void resize(const Mat& src, Mat dst, Size size, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR);
void copyMakeBorder(const Mat& src, Mat dst, int top, int bottom, int left, int right, int type);
void GaussianBlur(const Mat& src, Mat dst, Size ksize, double sigma_x, double sigma_y = 0, int border = BORDER_REFLECT_101);
class KeyPointsFilter {
 public:
  static void retainBest(std::vector<KeyPoint>&, int) { standin_not_provided("KeyPointsFilter::retainBest"); }
};

class FileNode {
 public:
  FileNode operator[](const std::string&) const { return fail(); }
  FileNode operator[](const char*) const { return fail(); }
  FileNode operator[](int) const { return fail(); }
  size_t size() const {
    fail();
    return 0;
  }
  operator int() const {
    fail();
    return 0;
  }
  operator float() const {
    fail();
    return 0.f;
  }
  operator double() const {
    fail();
    return 0.0;
  }
  operator std::string() const {
    fail();
    return std::string();
  }

 private:
  static FileNode fail() { throw std::runtime_error("cv stand-in: no file storage"); }
};

class FileStorage {
 public:
  enum Mode { READ = 0, WRITE = 1 };
  FileStorage() {}
  FileStorage(const std::string&, int) {}
  bool isOpened() const { return false; }
  FileNode operator[](const std::string&) const { throw std::runtime_error("cv stand-in: no file storage"); }
  FileNode operator[](const char*) const { throw std::runtime_error("cv stand-in: no file storage"); }
};

template <class T>
FileStorage& operator<<(FileStorage&, const T&) {
  throw std::runtime_error("cv stand-in: no file storage");
}

}  // namespace cv

#endif
