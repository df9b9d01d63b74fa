// sbm_stereosgbm.hpp -- header-only C++ adaptor that restores the cv::StereoSGBM spelling on top of the C-ABI (sbm.h,
// sbm_sgbm_*), so that the reference's second dense-disparity call site,
//
//     cv::Ptr<cv::StereoSGBM> sgbm = cv::StereoSGBM::create(-64, 128, 11, 100, 1000, 32, 0, 15, 1000, 16,
//                                                           cv::StereoSGBM::MODE_HH);          // src/slam/src/core/main.cpp:219-230
//     sgbm->compute(data.imageLeft(), data.imageRight(), disp);                                 // main.cpp:233
//
// compiles against the MI355X engine with a one-line type swap (sbm::StereoSGBM). create() takes the 11
// positional arguments with cv::StereoSGBM's defaults; setters and getters follow cv::StereoSGBM / cv::StereoMatcher.
// Failures throw from compute() (cv::Exception when OpenCV headers are present, sbm::Error otherwise). The destination is
// CV_16SC1 only (OpenCV's SGBM writes nothing else).
#ifndef SBM_STEREOSGBM_HPP_
#define SBM_STEREOSGBM_HPP_

#include "sbm_stereobm.hpp"   // sbm::Error and the OpenCV detection

namespace sbm {

class StereoSGBM {
 public:
  enum { MODE_SGBM = SBM_SGBM_MODE_SGBM, MODE_HH = SBM_SGBM_MODE_HH, MODE_SGBM_3WAY = SBM_SGBM_MODE_SGBM_3WAY,
         MODE_HH4 = SBM_SGBM_MODE_HH4 };

  // cv::StereoSGBM::create(minDisparity = 0, numDisparities = 16, blockSize = 3, P1 = 0, P2 = 0, disp12MaxDiff = 0,
  // preFilterCap = 0, uniquenessRatio = 0, speckleWindowSize = 0, speckleRange = 0, mode = MODE_SGBM); `device` selects
  // the HIP device (default 0).
  static std::shared_ptr<StereoSGBM> create(int minDisparity = 0, int numDisparities = 16, int blockSize = 3, int P1 = 0,
                                            int P2 = 0, int disp12MaxDiff = 0, int preFilterCap = 0, int uniquenessRatio = 0,
                                            int speckleWindowSize = 0, int speckleRange = 0, int mode = MODE_SGBM,
                                            int device = 0) {
    std::shared_ptr<StereoSGBM> m(new StereoSGBM(minDisparity, numDisparities, blockSize, device));
    m->p_.p1 = P1; m->p_.p2 = P2; m->p_.disp12_max_diff = disp12MaxDiff; m->p_.prefilter_cap = preFilterCap;
    m->p_.uniqueness_ratio = uniquenessRatio; m->p_.speckle_window_size = speckleWindowSize; m->p_.speckle_range = speckleRange;
    m->p_.mode = mode;
    return m;
  }

  ~StereoSGBM() { sbm_destroy(h_); }
  StereoSGBM(const StereoSGBM&) = delete;
  StereoSGBM& operator=(const StereoSGBM&) = delete;

  int getMinDisparity() const { return p_.min_disparity; }
  void setMinDisparity(int v) { p_.min_disparity = v; }
  int getNumDisparities() const { return p_.num_disparities; }
  void setNumDisparities(int v) { p_.num_disparities = v; }
  int getBlockSize() const { return p_.block_size; }
  void setBlockSize(int v) { p_.block_size = v; }
  int getP1() const { return p_.p1; }
  void setP1(int v) { p_.p1 = v; }
  int getP2() const { return p_.p2; }
  void setP2(int v) { p_.p2 = v; }
  int getDisp12MaxDiff() const { return p_.disp12_max_diff; }
  void setDisp12MaxDiff(int v) { p_.disp12_max_diff = v; }
  int getPreFilterCap() const { return p_.prefilter_cap; }
  void setPreFilterCap(int v) { p_.prefilter_cap = v; }
  int getUniquenessRatio() const { return p_.uniqueness_ratio; }
  void setUniquenessRatio(int v) { p_.uniqueness_ratio = v; }
  int getSpeckleWindowSize() const { return p_.speckle_window_size; }
  void setSpeckleWindowSize(int v) { p_.speckle_window_size = v; }
  int getSpeckleRange() const { return p_.speckle_range; }
  void setSpeckleRange(int v) { p_.speckle_range = v; }
  int getMode() const { return p_.mode; }
  void setMode(int v) { p_.mode = v; }

  // Raw-pointer compute: strides in bytes (cv::Mat::step). Output int16, 1/16 px, invalid = (minDisparity-1)*16.
  void compute(const uint8_t* left, size_t lstep, const uint8_t* right, size_t rstep, int width, int height, int16_t* disp,
               size_t dstep) {
    check(sbm_sgbm_compute(h_, &p_, left, lstep, right, rstep, width, height, disp, dstep));
  }

#ifdef SBM_HAVE_OPENCV
  // cv::StereoMatcher::compute(InputArray left, InputArray right, OutputArray disparity): CV_16SC1.
  void compute(cv::InputArray leftarr, cv::InputArray rightarr, cv::OutputArray disparr) {
    if (leftarr.size() != rightarr.size()) CV_Error(cv::Error::StsUnmatchedSizes, "All the images must have the same size");
    if (leftarr.type() != CV_8UC1 || rightarr.type() != CV_8UC1)
      CV_Error(cv::Error::StsUnsupportedFormat, "Both input images must have CV_8UC1");
    if (disparr.fixedType() && disparr.type() != CV_16SC1)
      CV_Error(cv::Error::StsUnsupportedFormat, "the SGBM disparity map is CV_16SC1");
    cv::Mat left = leftarr.getMat(), right = rightarr.getMat();
    disparr.create(left.size(), CV_16SC1);
    cv::Mat disp = disparr.getMat();
    int st = sbm_sgbm_compute(h_, &p_, left.ptr<uint8_t>(), left.step, right.ptr<uint8_t>(), right.step, left.cols, left.rows,
                              disp.ptr<int16_t>(), disp.step);
    if (st != SBM_OK) CV_Error(st <= SBM_ERR_NO_DEVICE ? cv::Error::StsError : cv::Error::StsOutOfRange, message(st));
  }
#endif

  sbm_handle* handle() const { return h_; }
  const sbm_sgbm_params& params() const { return p_; }

 private:
  StereoSGBM(int minDisparity, int numDisparities, int blockSize, int device) : h_(nullptr) {
    sbm_sgbm_params_default(&p_, minDisparity, numDisparities, blockSize);
    sbm_params bm;
    sbm_params_default(&bm, 0, 0);   // the handle's block-matcher parameters are not used by the SGBM entry points
    check(sbm_create(&h_, &bm, device));
  }
  std::string message(int st) const {
    std::string m = sbm_strerror(st);
    if (st == SBM_ERR_HIP) m += " (hipError " + std::to_string(sbm_last_hip_error(h_)) + ")";
    return m;
  }
  void check(int st) const {
    if (st != SBM_OK) throw Error(st, message(st));
  }
  sbm_sgbm_params p_;
  sbm_handle* h_;
};

}  // namespace sbm
#endif
