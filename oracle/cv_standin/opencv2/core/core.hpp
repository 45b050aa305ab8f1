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
//   cv::FAST, resize, copyMakeBorder, GaussianBlur, KeyPointsFilter: present
//                    so that the extractor's detection half compiles; every
//                    call throws - the pyramid, FAST, the octree and
//                    OpenCV's blur are not what is pinned
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
  static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }  // (a new store is value-initialised)
  static Mat zeros(Size s, int type) { return Mat(s, type); }
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
inline void FAST(const Mat&, std::vector<KeyPoint>&, int, bool = true) { standin_not_provided("FAST"); }
inline void resize(const Mat&, Mat, Size, double = 0, double = 0, int = INTER_LINEAR) { standin_not_provided("resize"); }
inline void copyMakeBorder(const Mat&, Mat, int, int, int, int, int) { standin_not_provided("copyMakeBorder"); }
inline void GaussianBlur(const Mat&, Mat, Size, double, double = 0, int = BORDER_REFLECT_101) { standin_not_provided("GaussianBlur"); }
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
