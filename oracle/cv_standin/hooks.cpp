// ============================================================================
// TEST INFRASTRUCTURE ONLY.  The four image functions of this project's OpenCV
// stand-in that the reference's ORB extractor calls in its detection half.
// FAST, resize and GaussianBlur are NOT implemented: each calls through a
// function pointer that a wrapper sets (oracle/orb_detect_ref.cpp hands the
// call to the test), and whose default throws "not provided" - so a library
// that sets none behaves as before.  copyMakeBorder is a simple rule and is
// implemented: BORDER_REFLECT_101, the source never read beyond its own range.
// ============================================================================
#include "opencv2/core/core.hpp"

namespace cv {
namespace {
void no_fast(const Mat&, std::vector<KeyPoint>&, int, bool) { standin_not_provided("FAST"); }
void no_resize(const Mat&, Mat&) { standin_not_provided("resize"); }
void no_blur(const Mat&, Mat&, int, double) { standin_not_provided("GaussianBlur"); }

// an output array created at rows x cols: as it lies where it has that size already, else not representable by a by-value Mat
void created(const Mat& dst, int rows, int cols, int type, const char* what) {
  if (dst.data == nullptr || dst.rows != rows || dst.cols != cols || dst.type() != type)
    throw std::runtime_error(std::string("cv stand-in: ") + what + " into a destination of another size or type is not provided");
}

// BORDER_REFLECT_101: gfedcb|abcdefgh|gfedcba
int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}
}  // namespace

standin_fast_fn standin_fast = no_fast;
standin_resize_fn standin_resize = no_resize;
standin_blur_fn standin_blur = no_blur;

void FAST(const Mat& image, std::vector<KeyPoint>& keypoints, int threshold, bool nonmax) {
  keypoints.clear();
  standin_fast(image, keypoints, threshold, nonmax);
}

void resize(const Mat& src, Mat dst, Size size, double fx, double fy, int interpolation) {
  if (interpolation != INTER_LINEAR || fx != 0 || fy != 0 || src.type() != CV_8U || src.empty() || size.width < 1 || size.height < 1)
    standin_not_provided("resize other than 8-bit INTER_LINEAR to a given size");
  created(dst, size.height, size.width, src.type(), "resize");
  standin_resize(src, dst);
}

void GaussianBlur(const Mat& src, Mat dst, Size ksize, double sigma_x, double sigma_y, int border) {
  if (border != BORDER_REFLECT_101 || ksize.width != ksize.height || (sigma_y != 0 && sigma_y != sigma_x) || src.type() != CV_8U || src.empty())
    standin_not_provided("GaussianBlur other than square, one sigma, 8-bit, BORDER_REFLECT_101");
  created(dst, src.rows, src.cols, src.type(), "GaussianBlur");
  const Mat copy = src.clone();  // (the reference blurs in place)
  standin_blur(copy, dst, ksize.width, sigma_x);
}

void copyMakeBorder(const Mat& src, Mat dst, int top, int bottom, int left, int right, int type) {
  if ((type & ~BORDER_ISOLATED) != BORDER_REFLECT_101 || src.type() != CV_8U || src.empty() || top < 0 || bottom < 0 || left < 0 || right < 0)
    standin_not_provided("copyMakeBorder other than 8-bit BORDER_REFLECT_101");
  const int rows = src.rows, cols = src.cols;
  created(dst, rows + top + bottom, cols + left + right, src.type(), "copyMakeBorder");
  // the interior, unless the destination already holds the source there as its own view
  if (src.data != dst.ptr(top) + left || src.step != dst.step)
    for (int r = 0; r < rows; ++r) std::memmove(dst.ptr(top + r) + left, src.ptr(r), (size_t)cols);
  // left and right of every interior row, from that row's interior
  for (int r = 0; r < rows; ++r) {
    unsigned char* row = dst.ptr(top + r);
    for (int c = 0; c < left; ++c) row[c] = row[left + reflect101(c - left, cols)];
    for (int c = 0; c < right; ++c) row[left + cols + c] = row[left + reflect101(cols + c, cols)];
  }
  // whole rows above and below, from the interior rows finished above
  for (int r = 0; r < top; ++r) std::memcpy(dst.ptr(r), dst.ptr(top + reflect101(r - top, rows)), (size_t)dst.cols);
  for (int r = 0; r < bottom; ++r) std::memcpy(dst.ptr(top + rows + r), dst.ptr(top + reflect101(rows + r, rows)), (size_t)dst.cols);
}
}  // namespace cv
