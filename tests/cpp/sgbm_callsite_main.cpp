// The reference's SGBM call site (src/slam/src/core/main.cpp:218-234) with the one-line type swap of INTEGRATION.md: a matcher
// created inside the frame loop with the 11 positional arguments of main.cpp:219-230 and one compute() (main.cpp:233). The
// frame comes from raw 8-bit files instead of cv::imread so that the program builds without OpenCV; with OpenCV headers present
// (-DSBM_TEST_WITH_OPENCV) the cv::InputArray / cv::OutputArray overload is what computes.
//
//   sgbm_callsite_main <left.raw> <right.raw> <width> <height> <disp_out.raw>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sbm_stereosgbm.hpp"

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]);
  const size_t npix = (size_t)W * H;
  std::vector<uint8_t> left(npix), right(npix);
  std::vector<int16_t> disp(npix);
  for (int k = 0; k < 2; k++) {
    FILE* f = std::fopen(argv[1 + k], "rb");
    if (!f) return 3;
    const size_t got = std::fread(k ? right.data() : left.data(), 1, npix, f);
    std::fclose(f);
    if (got != npix) return 3;
  }
  try {
    // --- main.cpp:219-230, cv::StereoSGBM -> sbm::StereoSGBM (the arguments positionally; their comments there are shifted)
    auto sgbm = sbm::StereoSGBM::create(-64, 128, 11, 100, 1000, 32, 0, 15, 1000, 16, sbm::StereoSGBM::MODE_HH);
    // --- main.cpp:233 ------------------------------------------------------------------------------------------------------
#ifdef SBM_TEST_WITH_OPENCV
    cv::Mat l(H, W, CV_8UC1, left.data()), r(H, W, CV_8UC1, right.data()), d;
    sgbm->compute(l, r, d);
    if (d.type() != CV_16SC1 || d.rows != H || d.cols != W) return 5;
    for (int y = 0; y < H; y++) std::copy(d.ptr<int16_t>(y), d.ptr<int16_t>(y) + W, disp.data() + (size_t)y * W);
#else
    sgbm->compute(left.data(), (size_t)W, right.data(), (size_t)W, W, H, disp.data(), (size_t)W * sizeof(int16_t));
#endif
  } catch (const sbm::Error& e) {
    std::printf("sbm::Error %d: %s\n", e.code, e.what());
    return 4;
  }
  FILE* f = std::fopen(argv[5], "wb");
  if (!f) return 6;
  const size_t put = std::fwrite(disp.data(), sizeof(int16_t), npix, f);
  std::fclose(f);
  return put == npix ? 0 : 6;
}
