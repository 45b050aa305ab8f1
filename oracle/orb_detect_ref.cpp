// ============================================================================
// TEST INFRASTRUCTURE ONLY.  Real-code oracle for the half of ORBextractor that
// gl_orb_pyramid and gl_orb_detect replace, and for the whole of detect().  It
// is linked into oracle/_ref/liborb_ref.so beside orb_ref.cpp, which #includes
// the reference's OWN gmmloc/src/cv/orb_extractor.cpp where it lies; this file
// sees the reference's class through its header alone.  Nothing of the
// reference is copied into this repository.
//
// What runs here is the reference's: the constructor's mnFeaturesPerLevel,
// ComputePyramid, ComputeKeyPointsOctTree, DistributeOctTree, DivideNode,
// computeOrientation behind them, and detect().  What is NOT: cv::FAST,
// cv::resize and cv::GaussianBlur - the stand-in hands each call to a callback
// of the test (cv_standin/hooks.cpp), so the reference's code AROUND them is
// pinned and their arithmetic is not - and copyMakeBorder, cvRound and the
// matrix, which are the stand-in's.
//
// `Pinned` derives from ORBextractor and adds access only.  Members that the
// constructor fixes and that set_levels() SETS, so that ComputeKeyPointsOctTree
// can run on levels the caller supplies: mvImagePyramid (views of caller
// memory), nlevels (1 .. 8, the length of the constructor's scale table),
// iniThFAST, minThFAST, mnFeaturesPerLevel.  Nothing else is written.
//
// A callback is a C function of the test's; it must not throw.  An exception of
// the stand-in (a range outside a matrix, a hook that was not set) is caught at
// the extern "C" boundary: the function returns -1 and orbref_last_error says
// what it was.
// ============================================================================
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "gmmloc/cv/orb_extractor.h"  // from -I$(REF)/gmmloc/include: the reference's header, where it lies

extern "C" {
// cv::FAST on the view [x0, x0 + cols) x [y0, y0 + rows) of level `level` (data / step: the view as the reference passed it):
// writes up to cap key-points as (x, y, response) in the VIEW's coordinates -> their number
typedef int (*orbref_fast_cb)(int level, int x0, int y0, const uint8_t* data, int64_t step, int cols, int rows, int threshold, int nonmax, int cap,
                              float* xyr);
typedef void (*orbref_resize_cb)(const uint8_t* src, int64_t src_step, int src_cols, int src_rows, uint8_t* dst, int64_t dst_step, int dst_cols,
                                 int dst_rows);
typedef void (*orbref_blur_cb)(const uint8_t* src, int64_t src_step, uint8_t* dst, int64_t dst_step, int cols, int rows, int ksize, double sigma);
}

namespace {
const int EDGE = 19;  // EDGE_THRESHOLD of orb_extractor.cpp:75 (file-local there); orbref_pyramid_info reports what the reference did with it

struct Pinned : public gmmloc::ORBextractor {
  explicit Pinned(int nfeatures) : ORBextractor(nfeatures) {}
  const std::vector<int>& per_level() const { return mnFeaturesPerLevel; }
  int levels() const { return nlevels; }
  void pyramid(const cv::Mat& image) { ComputePyramid(image); }
  void key_points(std::vector<std::vector<cv::KeyPoint>>& all) { ComputeKeyPointsOctTree(all); }
  std::vector<cv::KeyPoint> distribute(const std::vector<cv::KeyPoint>& keys, int min_x, int max_x, int min_y, int max_y, int n) {
    return DistributeOctTree(keys, min_x, max_x, min_y, max_y, n, 0);
  }
  void set_levels(const std::vector<cv::Mat>& views, int ini_th, int min_th, const int32_t* per_level) {
    mvImagePyramid = views;
    nlevels = (int)views.size();
    iniThFAST = ini_th;
    minThFAST = min_th;
    mnFeaturesPerLevel.assign(per_level, per_level + views.size());
  }
};

std::unique_ptr<Pinned> ext;  // the extractor that the pyramid / key-point calls share
std::string last_error;
struct FastCall {
  int32_t level, x0, y0, cols, rows, threshold, nonmax;
};
std::vector<FastCall> fast_calls;
orbref_fast_cb fast_cb = nullptr;
orbref_resize_cb resize_cb = nullptr;
orbref_blur_cb blur_cb = nullptr;

void hook_fast(const cv::Mat& image, std::vector<cv::KeyPoint>& keypoints, int threshold, bool nonmax) {
  FastCall c{-1, 0, 0, image.cols, image.rows, threshold, nonmax ? 1 : 0};
  if (ext)
    for (int l = 0; l < (int)ext->mvImagePyramid.size(); ++l) {  // which level holds the view, and where
      const cv::Mat& m = ext->mvImagePyramid[l];
      if (m.empty() || image.step != m.step || image.data < m.data) continue;
      const size_t off = (size_t)(image.data - m.data);
      if (off / m.step < (size_t)m.rows && off % m.step < (size_t)m.cols) {
        c.level = l, c.y0 = (int)(off / m.step), c.x0 = (int)(off % m.step);
        break;
      }
    }
  fast_calls.push_back(c);
  if (!fast_cb) return;
  const int cap = image.rows * image.cols;
  std::vector<float> xyr((size_t)cap * 3 + 3);
  int n = fast_cb(c.level, c.x0, c.y0, image.data, (int64_t)image.step, image.cols, image.rows, threshold, c.nonmax, cap, xyr.data());
  if (n > cap) n = cap;
  for (int i = 0; i < n; ++i) keypoints.push_back(cv::KeyPoint(xyr[3 * i], xyr[3 * i + 1], 7.f, -1.f, xyr[3 * i + 2]));  // (7: what cv::FAST sets as size)
}

void hook_resize(const cv::Mat& src, cv::Mat& dst) {
  if (!resize_cb) cv::standin_not_provided("resize (no callback set)");
  resize_cb(src.data, (int64_t)src.step, src.cols, src.rows, dst.data, (int64_t)dst.step, dst.cols, dst.rows);
}

void hook_blur(const cv::Mat& src, cv::Mat& dst, int ksize, double sigma) {
  if (!blur_cb) cv::standin_not_provided("GaussianBlur (no callback set)");
  blur_cb(src.data, (int64_t)src.step, dst.data, (int64_t)dst.step, src.cols, src.rows, ksize, sigma);
}

template <class F>
int guarded(F f) {
  try {
    last_error.clear();
    return f();
  } catch (const std::exception& e) {
    last_error = e.what();
  } catch (...) {
    last_error = "unknown exception";
  }
  return -1;
}

void put(const cv::KeyPoint& k, float* out) {
  out[0] = k.pt.x, out[1] = k.pt.y, out[2] = (float)k.octave, out[3] = k.size, out[4] = k.response, out[5] = k.angle;
}
}  // namespace

extern "C" {
const char* orbref_last_error() { return last_error.c_str(); }

// the callbacks (NULL: FAST finds nothing; resize / GaussianBlur throw "not provided").  Sets the stand-in's pointers.
void orbref_set_hooks(orbref_fast_cb fast, orbref_resize_cb resize, orbref_blur_cb blur) {
  fast_cb = fast, resize_cb = resize, blur_cb = blur;
  cv::standin_fast = hook_fast, cv::standin_resize = hook_resize, cv::standin_blur = hook_blur;
}

// the record of the FAST calls since the last orbref_fast_reset, in order: 7 ints each {level, x0, y0, cols, rows, threshold, nonmax}
// -> their number (all of them, whatever cap is)
int orbref_fast_calls(int32_t* out, int cap) {
  for (int i = 0; i < (int)fast_calls.size() && i < cap; ++i) std::memcpy(out + 7 * i, &fast_calls[i], sizeof(FastCall));
  return (int)fast_calls.size();
}
void orbref_fast_reset() { fast_calls.clear(); }

// mnFeaturesPerLevel [8] of an extractor constructed with nfeatures -> nlevels
int orbref_features_per_level(int nfeatures, int32_t* per_level) {
  return guarded([&] {
    Pinned p(nfeatures);
    for (size_t i = 0; i < p.per_level().size() && i < 8; ++i) per_level[i] = p.per_level()[i];
    return (int)p.per_level().size();
  });
}

// DistributeOctTree on n keys (x, y, response) relative to (min_x, min_y) -> vResultKeys in order as (x, y, response), up to cap; the
// return value is their number
int orbref_distribute(const float* keys, int n, int min_x, int max_x, int min_y, int max_y, int N, float* out, int cap) {
  return guarded([&] {
    Pinned p(N);
    std::vector<cv::KeyPoint> in;
    for (int i = 0; i < n; ++i) in.push_back(cv::KeyPoint(keys[3 * i], keys[3 * i + 1], 7.f, -1.f, keys[3 * i + 2]));
    const std::vector<cv::KeyPoint> res = p.distribute(in, min_x, max_x, min_y, max_y, N);
    for (int i = 0; i < (int)res.size() && i < cap; ++i) out[3 * i] = res[i].pt.x, out[3 * i + 1] = res[i].pt.y, out[3 * i + 2] = res[i].response;
    return (int)res.size();
  });
}

// a new extractor(nfeatures) and ComputePyramid on the caller's image -> nlevels
int orbref_pyramid(const uint8_t* img, int width, int height, int64_t stride, int nfeatures) {
  return guarded([&] {
    ext.reset(new Pinned(nfeatures));
    ext->pyramid(cv::Mat(height, width, CV_8UC1, const_cast<uint8_t*>(img), (size_t)stride));
    return ext->levels();
  });
}

// per level of the shared extractor, 6 ints: {rows, cols, step, the view's byte offset inside the matrix it was cut from (`temp`), that
// matrix's size in bytes, 0} -> the number of levels.  (Levels set by orbref_set_levels are caller memory: offset and size 0.)
int orbref_pyramid_info(int32_t* info) {
  return guarded([&] {
    if (!ext) throw std::runtime_error("no extractor");
    const std::vector<cv::Mat>& py = ext->mvImagePyramid;
    for (size_t l = 0; l < py.size(); ++l) {
      const cv::Mat& m = py[l];
      const unsigned char* base = m.standin_store_begin();
      const int32_t row[6] = {m.rows, m.cols, (int32_t)m.step, base ? (int32_t)(m.data - base) : 0, (int32_t)m.standin_store_size(), 0};
      std::memcpy(info + 6 * l, row, sizeof(row));
    }
    return (int)py.size();
  });
}

// the pixels of a level of the shared extractor: whole = 0: the view, rows x cols; whole = 1: the matrix it was cut from, store size bytes
int orbref_level_pixels(int level, int whole, uint8_t* out) {
  return guarded([&] {
    if (!ext || level < 0 || level >= (int)ext->mvImagePyramid.size()) throw std::runtime_error("no such level");
    const cv::Mat& m = ext->mvImagePyramid[level];
    if (whole) {
      if (!m.standin_store_begin()) throw std::runtime_error("the level is caller memory");
      std::memcpy(out, m.standin_store_begin(), m.standin_store_size());
    } else
      for (int r = 0; r < m.rows; ++r) std::memcpy(out + (size_t)r * m.cols, m.ptr(r), (size_t)m.cols);
    return 0;
  });
}

// overwrites every byte of every level's own matrix that lies OUTSIDE the level's view (the 19 px border of :1061-1077) with
// (seed + 37 i) mod 256, i the byte's index -> the number of bytes written
int orbref_overwrite_borders(int seed) {
  return guarded([&] {
    if (!ext) throw std::runtime_error("no extractor");
    int written = 0;
    for (const cv::Mat& m : ext->mvImagePyramid) {
      unsigned char* base = const_cast<unsigned char*>(m.standin_store_begin());
      if (!base) throw std::runtime_error("the level is caller memory");
      const size_t off = (size_t)(m.data - base), size = m.standin_store_size();
      for (size_t i = 0; i < size; ++i) {
        const bool inside = i >= off && (i - off) / m.step < (size_t)m.rows && (i - off) % m.step < (size_t)m.cols;
        if (!inside) base[i] = (unsigned char)(seed + 37 * i), ++written;
      }
    }
    return written;
  });
}

// a new extractor(nfeatures) whose pyramid is the caller's levels (views: the memory must outlive the key-point call), with the
// thresholds and the per-level counts given: the members named in this file's header are SET
int orbref_set_levels(int nfeatures, int nlevels, const uint8_t* const* data, const int32_t* width, const int32_t* height, const int64_t* stride,
                      int ini_th, int min_th, const int32_t* per_level) {
  return guarded([&] {
    if (nlevels < 1 || nlevels > 8) throw std::runtime_error("1 .. 8 levels");
    ext.reset(new Pinned(nfeatures));
    std::vector<cv::Mat> views;
    for (int l = 0; l < nlevels; ++l) views.push_back(cv::Mat(height[l], width[l], CV_8UC1, const_cast<uint8_t*>(data[l]), (size_t)stride[l]));
    ext->set_levels(views, ini_th, min_th, per_level);
    return nlevels;
  });
}

// ComputeKeyPointsOctTree on the shared extractor's pyramid -> allKeypoints: level_count [8], and level by level up to cap key-points of
// 6 floats {pt.x, pt.y, octave, size, response, angle}; the return value is their number
int orbref_key_points(int32_t* level_count, float* kp, int cap) {
  return guarded([&] {
    if (!ext) throw std::runtime_error("no extractor");
    std::vector<std::vector<cv::KeyPoint>> all;
    ext->key_points(all);
    int n = 0;
    for (int l = 0; l < 8; ++l) level_count[l] = l < (int)all.size() ? (int)all[l].size() : 0;
    for (const auto& level : all)
      for (const cv::KeyPoint& k : level) {
        if (n < cap) put(k, kp + 6 * n);
        ++n;
      }
    return n;
  });
}

// a new extractor(nfeatures) and the whole detect() on the caller's image -> _keypoints (6 floats each as above, pt after `*= scale`)
// and _descriptors (32 bytes each), up to cap; the return value is their number.  The extractor stays the shared one.
int orbref_detect(const uint8_t* img, int width, int height, int64_t stride, int nfeatures, float* kp, uint8_t* desc, int cap) {
  return guarded([&] {
    ext.reset(new Pinned(nfeatures));
    std::vector<cv::KeyPoint> keys;
    cv::Mat descriptors;
    ext->detect(cv::Mat(height, width, CV_8UC1, const_cast<uint8_t*>(img), (size_t)stride), cv::Mat(), keys, descriptors);
    if (!keys.empty() && (descriptors.rows != (int)keys.size() || descriptors.cols != 32)) throw std::runtime_error("descriptors' shape");
    for (int i = 0; i < (int)keys.size() && i < cap; ++i) {
      put(keys[i], kp + 6 * i);
      std::memcpy(desc + (size_t)32 * i, descriptors.ptr(i), 32);
    }
    return (int)keys.size();
  });
}
}
