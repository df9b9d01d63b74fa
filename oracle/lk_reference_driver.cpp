// lk_reference_driver.cpp -- our half of oracle/_ref/liblk_reference.so. The other half is the reference's own
// calcOpticalFlowPyrLKStereo (src/slam/src/opencv/CvLKStereo.cpp), compiled from the reference tree as it stands against the
// OpenCV stand-in of tests/cpp/mock_opencv (oracle/Makefile). TEST INFRASTRUCTURE ONLY.
//
// What this file does: it takes the unpadded pyramid levels and derivative planes of one pair (from lk_stereo_ref.pyramid: the
// pyramid stays RECALLED, this build pins the tracker GIVEN the pyramid), lays each plane out as cv::buildOpticalFlowPyramid
// would -- a rectangle inside a plane padded by winSize on every side, the image padded with BORDER_REFLECT_101, the derivative
// with zeros -- and calls the tracker with the two level-0 images, as computeCorrespondences does. The tracker then asks
// cv::buildOpticalFlowPyramid for the pyramids; the definition below computes nothing and hands back the prepared planes,
// interleaved [level, deriv] when withDerivatives is set. The tracker reads real padded memory, the engine applies the border
// rule at the read: the comparison holds that equivalence too.
// Build: oracle/Makefile (-O2 -std=c++17 -fPIC -ffp-contract=off).
#include <cstdarg>
#include <cstdint>
#include <vector>

#include "core/Logger.h"
#include "opencv/CvLKStereo.h"

// the reference's logger, which the tracker calls once (an empty-matrix warning); nothing is logged here
void log_write(LOG_LEVEL, const char*, int, const char*, const char*, ...) {}

namespace {

struct Prepared {
  const void* key = nullptr;                 // data pointer of the level-0 image the tracker passes on
  std::vector<cv::Mat> levels, derivs;       // rectangles inside the padded planes below
  std::vector<std::vector<unsigned char>> planes;
  std::vector<std::vector<short>> dplanes;
};
Prepared* g_prepared[2] = {nullptr, nullptr};

int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

// flat: the unpadded levels back to back, level 0 first; dflat (may be null): the same order in (dx, dy) pairs
void prepare(Prepared& p, const unsigned char* flat, const short* dflat, const int* lw, const int* lh, int nlevels, int ww, int wh) {
  size_t off = 0;
  for (int l = 0; l < nlevels; l++) {
    const int w = lw[l], h = lh[l], pw = w + 2 * ww, ph = h + 2 * wh;
    p.planes.emplace_back((size_t)pw * ph);
    unsigned char* d = p.planes.back().data();
    for (int y = 0; y < ph; y++)
      for (int x = 0; x < pw; x++) d[(size_t)y * pw + x] = flat[off + (size_t)reflect101(y - wh, h) * w + reflect101(x - ww, w)];
    p.levels.push_back(cv::Mat(ph, pw, CV_8UC1, d)(cv::Rect(ww, wh, w, h)));
    if (dflat) {
      p.dplanes.emplace_back((size_t)pw * ph * 2, (short)0);
      short* dd = p.dplanes.back().data();
      for (int y = 0; y < h; y++)
        for (int x = 0; x < 2 * w; x++) dd[((size_t)(y + wh) * pw + ww) * 2 + x] = dflat[2 * off + (size_t)y * 2 * w + x];
      p.derivs.push_back(cv::Mat(ph, pw, CV_16SC2, dd)(cv::Rect(ww, wh, w, h)));
    }
    off += (size_t)w * h;
  }
  p.key = p.levels[0].ptr();
}

}  // namespace

namespace cv {

int buildOpticalFlowPyramid(InputArray img, std::vector<Mat>& pyramid, Size, int maxLevel, bool withDerivatives) {
  const Mat m = img.getMat();
  const Prepared* p = nullptr;
  for (Prepared* q : g_prepared)
    if (q && q->key == m.ptr()) p = q;
  CV_Assert(p != nullptr && (!withDerivatives || p->derivs.size() == p->levels.size()));
  const int last = std::min(maxLevel, (int)p->levels.size() - 1);
  pyramid.clear();
  for (int l = 0; l <= last; l++) {
    pyramid.push_back(p->levels[l]);
    if (withDerivatives) pyramid.push_back(p->derivs[l]);
  }
  return last;
}

}  // namespace cv

// criteria_type: cv::TermCriteria's type bits (COUNT = 1, EPS = 2; computeCorrespondences sets both). Returns 0, or -1 where the
// tracker threw (an assertion of the reference's or of the stand-in's).
extern "C" int lk_reference_track(const unsigned char* left, const unsigned char* right, const short* deriv, const int* lw, const int* lh,
                                  int nlevels, const float* pts, int n, int win_w, int win_h, int max_level, int criteria_type,
                                  int max_count, double epsilon, int flags, double min_eig_threshold, float* out,
                                  unsigned char* status, float* err) {
  Prepared L, R;
  try {
    prepare(L, left, deriv, lw, lh, nlevels, win_w, win_h);
    prepare(R, right, nullptr, lw, lh, nlevels, win_w, win_h);
    g_prepared[0] = &L;
    g_prepared[1] = &R;
    cv::Mat prev((int)n, 1, CV_32FC2, const_cast<float*>(pts)), next, st, er;
    calcOpticalFlowPyrLKStereo(L.levels[0], R.levels[0], prev, next, st, er, cv::Size(win_w, win_h), max_level,
                               cv::TermCriteria(criteria_type, max_count, epsilon), flags, min_eig_threshold);
    g_prepared[0] = g_prepared[1] = nullptr;
    if (n > 0) {
      CV_Assert(next.checkVector(2, CV_32F, true) == n && st.checkVector(1, CV_8U, true) == n && er.checkVector(1, CV_32F, true) == n);
      for (int i = 0; i < n; i++) {
        out[2 * i] = next.ptr<cv::Point2f>()[i].x;
        out[2 * i + 1] = next.ptr<cv::Point2f>()[i].y;
        status[i] = st.ptr()[i];
        err[i] = er.ptr<float>()[i];
      }
    }
    return 0;
  } catch (const cv::Exception&) {
    g_prepared[0] = g_prepared[1] = nullptr;
    return -1;
  }
}
