// ============================================================================
// TEST INFRASTRUCTURE ONLY.  This project's own stand-in for the one OpenCV
// header the reference's DBoW2 includes, written from scratch: a byte matrix
// and a file storage that cannot be opened.  It exists so that
// oracle/dbow2_ref.cpp can compile the reference's vocabulary code where it
// lies; nothing of the product includes it.
//   cv::Mat          row-major bytes, shared on copy, deep on clone()
//   cv::FileStorage  present so that the YAML save / load members compile:
//   cv::FileNode     never open, every use throws
// The standard headers at the end of the list are the ones the reference's
// header expects to arrive with this one (pow, log, memcpy, stringstream).
// ============================================================================
#ifndef GMMLOC_ORACLE_CV_STANDIN_CORE_HPP
#define GMMLOC_ORACLE_CV_STANDIN_CORE_HPP

#include <cstddef>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <math.h>
#include <string.h>
#include <cmath>
#include <cstring>
#include <iostream>
#include <sstream>

#define CV_8U 0
#define CV_32F 5

namespace cv {

class Mat {
 public:
  int rows = 0, cols = 0;
  unsigned char* data = nullptr;

  Mat() {}
  Mat(int r, int c, int type) { create(r, c, type); }

  void create(int r, int c, int type) {
    const size_t bytes = (size_t)r * (size_t)c * elem_size(type);
    if (store_ && r == rows && c == cols && type == type_) return;
    store_ = std::make_shared<std::vector<unsigned char>>(bytes);
    rows = r, cols = c, type_ = type;
    data = store_->data();
  }
  static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }  // (a new store is value-initialised)
  Mat clone() const {
    Mat m;
    if (store_) {
      m.store_ = std::make_shared<std::vector<unsigned char>>(*store_);
      m.rows = rows, m.cols = cols, m.type_ = type_;
      m.data = m.store_->data();
    }
    return m;
  }
  void release() {
    store_.reset();
    rows = cols = 0;
    data = nullptr;
  }
  bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
  template <class T>
  T* ptr(int row = 0) {
    return reinterpret_cast<T*>(data + (size_t)row * (size_t)cols * elem_size(type_));
  }
  template <class T>
  const T* ptr(int row = 0) const {
    return reinterpret_cast<const T*>(data + (size_t)row * (size_t)cols * elem_size(type_));
  }

 private:
  static size_t elem_size(int type) {
    if (type == CV_8U) return 1;
    if (type == CV_32F) return 4;
    throw std::runtime_error("cv stand-in: element type not provided");
  }
  std::shared_ptr<std::vector<unsigned char>> store_;
  int type_ = CV_8U;
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
