// What the drivers of tests/cpp/ share: the model preamble, reading and writing the binary scene / result files, and moving a vector to
// the device and back through the C-ABI.  Plain C++17; templates or inline, so a driver may use any part of it.
#pragma once

#include <fstream>
#include <iostream>
#include <vector>

#include "gmmloc_hip/gmm_adapter.hpp"

// the model file into `model`; on failure the loader's message on stderr ("loadGMMModel: ..."), and the driver returns 1
inline bool load_model(const char* path, gmmloc_hip::GMM& model) {
  if (gmmloc_hip::GMM::loadGMMModel(path, model)) return true;
  std::cerr << "loadGMMModel: " << gmmloc_hip::GMM::last_error() << "\n";
  return false;
}

template <class T>
std::vector<T> rd(std::ifstream& f, size_t n) {
  std::vector<T> v(n);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
  return v;
}
template <class T>
void wr(std::ofstream& f, const std::vector<T>& v) {
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}
template <class T>
T* up(gl_ctx_t* ctx, const std::vector<T>& v) {
  void* p = nullptr;
  gmmloc_hip::check(gl_malloc(ctx, v.size() * sizeof(T) + 8, &p), "gl_malloc");
  if (!v.empty()) gmmloc_hip::check(gl_memcpy_h2d(ctx, p, v.data(), v.size() * sizeof(T)), "h2d");
  return static_cast<T*>(p);
}
template <class T>
std::vector<T> down(gl_ctx_t* ctx, const T* p, size_t n) {
  std::vector<T> v(n);
  if (n) gmmloc_hip::check(gl_memcpy_d2h(ctx, v.data(), p, n * sizeof(T)), "d2h");
  return v;
}
