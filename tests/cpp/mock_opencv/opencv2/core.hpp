// tests/cpp/mock_opencv/opencv2/core.hpp -- a MOCK of the handful of OpenCV core names that the cv:: overloads of
// include/sbm_*.hpp and the call-site programs of tests/cpp/ use.  Test infrastructure only.
//
// Written from scratch from the list of names those overloads touch (cv::Mat, cv::Mat_<T>, cv::Rect, cv::Size,
// cv::InputArray / cv::OutputArray with getMat / create / fixedType / type / size, Mat::convertTo, CV_Error,
// cv::Exception, the few names of the feature call sites, each in a section of its own at the end, and the small surface the
// reference's own LK tracker touches: ROI views with locateROI, Point_, TermCriteria, AutoBuffer, cvFloor / cvRound, CV_Assert);
// it is not derived from OpenCV's headers and reproduces none of OpenCV's arithmetic beyond the documented meaning of
// cvFloor, cvRound and the Point_ operators.  What it is for:
// this image (and the GPU box) has no OpenCV, so the overload the maintainer's one-line diff at
// src/slam/src/core/main.cpp:201-215 relies on had never been through a compiler.  Building against this mock proves that
// text compiles and runs -- the call shape, the CV_16SC1 / fixed-CV_32F destination rule, the error -> cv::Exception
// mapping.  It pins NOTHING about cv::StereoBM's results or any other OpenCV arithmetic; where real OpenCV headers exist
// the test uses those instead.
#ifndef SBM_MOCK_OPENCV_CORE_HPP_
#define SBM_MOCK_OPENCV_CORE_HPP_

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#define SBM_MOCK_OPENCV 1

// type codes: depth in the low 3 bits, (channels - 1) above them -- the call sites use the three single-channel types below, the
// tracker section at the end the two-channel ones as well
#define CV_8U 0
#define CV_16S 3
#define CV_32F 5
#define CV_MAKETYPE(depth, cn) (((depth) & 7) + (((cn) - 1) << 3))
#define CV_8UC1 CV_8U
#define CV_16SC1 CV_16S
#define CV_32FC1 CV_32F
#define CV_16SC2 CV_MAKETYPE(CV_16S, 2)
#define CV_32FC2 CV_MAKETYPE(CV_32F, 2)

typedef unsigned char uchar;

namespace cv {

namespace Error {
enum Code { StsError = -2, StsOutOfRange = -211, StsUnmatchedSizes = -209, StsUnsupportedFormat = -210, StsAssert = -215 };
}

class Exception : public std::exception {
 public:
  Exception(int c, const std::string& m) : code(c), err(m) {}
  const char* what() const noexcept override { return err.c_str(); }
  int code;
  std::string err;
};

struct Size {
  int width, height;
  Size() : width(0), height(0) {}
  Size(int w, int h) : width(w), height(h) {}
  bool operator==(const Size& o) const { return width == o.width && height == o.height; }
  bool operator!=(const Size& o) const { return !(*this == o); }
  int area() const { return width * height; }
};

// cv::Point_<T> with the operators OpenCV documents for it: componentwise, every result converted back to T; ddot in double
template <class T>
struct Point_ {
  T x, y;
  Point_() : x(0), y(0) {}
  Point_(T x_, T y_) : x(x_), y(y_) {}
  Point_& operator+=(const Point_& o) { x = (T)(x + o.x); y = (T)(y + o.y); return *this; }
  Point_& operator-=(const Point_& o) { x = (T)(x - o.x); y = (T)(y - o.y); return *this; }
  double ddot(const Point_& o) const { return (double)x * o.x + (double)y * o.y; }
};
template <class T> inline Point_<T> operator+(const Point_<T>& a, const Point_<T>& b) { return Point_<T>((T)(a.x + b.x), (T)(a.y + b.y)); }
template <class T> inline Point_<T> operator-(const Point_<T>& a, const Point_<T>& b) { return Point_<T>((T)(a.x - b.x), (T)(a.y - b.y)); }
template <class T> inline Point_<T> operator*(const Point_<T>& a, float b) { return Point_<T>((T)(a.x * b), (T)(a.y * b)); }
typedef Point_<int> Point2i;
typedef Point2i Point;
typedef Point_<float> Point2f;

struct Rect {
  int x, y, width, height;
  Rect() : x(0), y(0), width(0), height(0) {}
  Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};

class _OutputArray;

// dense row-major matrix: either a view of caller memory or the owner of a shared buffer. A view may be a rectangle inside a
// larger plane (operator()(Rect)): step stays the plane's, and locateROI answers where the rectangle lies in it
class Mat {
 public:
  struct Step {   // converts like cv::MatStep: bytes per row
    size_t v = 0;
    operator size_t() const { return v; }
  };
  int rows = 0, cols = 0;
  Step step;
  Mat() {}
  Mat(int r, int c, int type, void* external, size_t step_bytes = 0)
      : rows(r), cols(c), type_(type), data_(static_cast<unsigned char*>(external)), whole_(c, r) {
    step.v = step_bytes ? step_bytes : (size_t)c * esz(type);
  }
  Mat(Size s, int type, void* external, size_t step_bytes = 0) : Mat(s.height, s.width, type, external, step_bytes) {}
  static size_t esz1(int type) { return (type & 7) == CV_8U ? 1 : ((type & 7) == CV_16S ? 2 : 4); }
  static size_t esz(int type) { return esz1(type) * (size_t)((type >> 3) + 1); }
  int type() const { return type_; }
  int depth() const { return type_ & 7; }
  int channels() const { return (type_ >> 3) + 1; }
  size_t elemSize1() const { return esz1(type_); }
  size_t total() const { return (size_t)rows * cols; }
  bool isContinuous() const { return rows <= 1 || step.v == (size_t)cols * esz(type_); }
  Size size() const { return Size(cols, rows); }
  bool empty() const { return data_ == nullptr; }
  void create(Size s, int type) {
    if (data_ && rows == s.height && cols == s.width && type_ == type) return;
    own_ = std::make_shared<std::vector<unsigned char>>((size_t)s.width * s.height * esz(type));
    data_ = own_->data(); rows = s.height; cols = s.width; type_ = type; step.v = (size_t)s.width * esz(type);
    whole_ = s; ofs_x_ = ofs_y_ = 0;
  }
  void release() { own_.reset(); data_ = nullptr; rows = cols = 0; step.v = 0; whole_ = Size(); ofs_x_ = ofs_y_ = 0; }
  void create(int r, int c, int type) { create(Size(c, r), type); }
  template <class T> T* ptr(int r = 0) { return reinterpret_cast<T*>(data_ + (size_t)r * step.v); }
  template <class T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(data_ + (size_t)r * step.v); }
  uchar* ptr(int r = 0) { return data_ + (size_t)r * step.v; }
  const uchar* ptr(int r = 0) const { return data_ + (size_t)r * step.v; }
  // the rectangle r of this matrix, sharing its memory
  Mat operator()(const Rect& r) const {
    Mat m(*this);
    m.data_ = data_ + (size_t)r.y * step.v + (size_t)r.x * esz(type_);
    m.rows = r.height; m.cols = r.width; m.ofs_x_ = ofs_x_ + r.x; m.ofs_y_ = ofs_y_ + r.y;
    return m;
  }
  // size of the plane this matrix is a rectangle of, and the rectangle's corner in it
  void locateROI(Size& whole, Point& ofs) const { whole = whole_; ofs = Point(ofs_x_, ofs_y_); }
  // the number of elemChannels-tuples of the given depth this matrix holds as a vector (1 x N or N x 1 with elemChannels
  // channels, or N x elemChannels with one channel), or -1 where it is no such vector
  int checkVector(int elemChannels, int depth = -1, bool requireContinuous = true) const {
    if ((depth >= 0 && this->depth() != depth) || (requireContinuous && !isContinuous())) return -1;
    if (channels() == elemChannels && (rows == 1 || cols == 1)) return rows * cols;
    if (channels() == 1 && cols == elemChannels) return rows;
    return -1;
  }
  // only the conversion the adaptor needs: CV_16S -> CV_32F with a scale factor
  inline void convertTo(const _OutputArray& dst, int rtype, double alpha = 1.0) const;

 protected:
  int type_ = CV_8U;
  unsigned char* data_ = nullptr;
  std::shared_ptr<std::vector<unsigned char>> own_;
  Size whole_;
  int ofs_x_ = 0, ofs_y_ = 0;
};

// matrix with a compile-time element type: as an output argument its type is FIXED
template <class T> struct MatTypeOf;
template <> struct MatTypeOf<unsigned char> { enum { value = CV_8U }; };
template <> struct MatTypeOf<short> { enum { value = CV_16S }; };
template <> struct MatTypeOf<float> { enum { value = CV_32F }; };
template <class T>
class Mat_ : public Mat {
 public:
  Mat_() { type_ = MatTypeOf<T>::value; }
  Mat_(int r, int c) { type_ = MatTypeOf<T>::value; create(r, c, MatTypeOf<T>::value); }
};

class _InputArray {
 public:
  enum { NONE = 0, MAT = 1 << 16, STD_VECTOR_MAT = 5 << 16 };
  _InputArray(const Mat& m) : m_(const_cast<Mat*>(&m)) {}   // NOLINT: implicit, like cv::InputArray
  _InputArray(const std::vector<Mat>& v) : m_(nullptr), v_(&v) {}   // NOLINT
  Size size() const { return m_->size(); }
  int type() const { return m_->type(); }
  Mat getMat() const { return *m_; }
  int kind() const { return v_ ? STD_VECTOR_MAT : MAT; }
  void getMatVector(std::vector<Mat>& out) const { if (v_) out = *v_; else out.clear(); }

 protected:
  Mat* m_;
  const std::vector<Mat>* v_ = nullptr;
};

class _OutputArray : public _InputArray {
 public:
  _OutputArray(Mat& m) : _InputArray(m), fixed_(false) {}   // NOLINT
  template <class T> _OutputArray(Mat_<T>& m) : _InputArray(m), fixed_(true) {}   // NOLINT
  bool fixedType() const { return fixed_; }
  // i (the index into a vector of matrices) and allowTransposed are accepted and have no meaning for a single matrix
  void create(Size s, int type, int i = -1, bool allowTransposed = false) const {
    (void)i; (void)allowTransposed;
    if (fixed_ && type != m_->type()) throw Exception(Error::StsUnsupportedFormat, "mock: a fixed-type destination cannot change its type");
    m_->create(s, type);
  }
  void create(int rows, int cols, int type, int i = -1, bool allowTransposed = false) const { create(Size(cols, rows), type, i, allowTransposed); }
  void release() const { m_->release(); }
  bool needed() const { return m_ != nullptr; }

 private:
  bool fixed_;
};

class _InputOutputArray : public _OutputArray {
 public:
  _InputOutputArray(Mat& m) : _OutputArray(m) {}   // NOLINT
};

typedef const _InputArray& InputArray;
typedef const _OutputArray& OutputArray;
typedef const _InputOutputArray& InputOutputArray;

inline void Mat::convertTo(const _OutputArray& dst, int rtype, double alpha) const {
  if (type_ != CV_16S || rtype != CV_32F) throw Exception(Error::StsUnsupportedFormat, "mock: only CV_16S -> CV_32F is implemented");
  dst.create(size(), CV_32F);
  Mat out = dst.getMat();
  for (int y = 0; y < rows; y++) {
    const short* s = ptr<short>(y);
    float* d = out.ptr<float>(y);
    for (int x = 0; x < cols; x++) d[x] = (float)(s[x] * alpha);
  }
}

// ---- keypoint call sites (include/sbm_gftt.hpp's reference-signature overload): cv::Point2f and cv::KeyPoint, written from
// the constructor the reference calls (cv::KeyPoint(pt, size), GFTT.cpp:166), with OpenCV's documented defaults for the other
// fields (cv::Point2f is Point_<float>, above)

struct KeyPoint {
  Point2f pt;
  float size = 0.f, angle = -1.f, response = 0.f;
  int octave = 0, class_id = -1;
  KeyPoint() {}
  KeyPoint(Point2f p, float s, float a = -1.f, float r = 0.f, int o = 0, int c = -1)
      : pt(p), size(s), angle(a), response(r), octave(o), class_id(c) {}
};

// ---- descriptor call site (computeDescriptor(image, cv::noArray(), kpts2d, true, desc), main.cpp:246-248): cv::noArray()
inline InputArray noArray() {
  static Mat empty;
  static _InputArray a(empty);
  return a;
}

// ---- matching call site (matchingGuess's kptsFrom3D, Registration.cpp:250-303): cv::Point3f. The motion-estimation call site
// (estimateMotion3DTo2D's std::map<int, cv::Point3f> and std::map<int, cv::KeyPoint>, Registration.cpp:337-397) adds no name
struct Point3f {
  float x = 0.f, y = 0.f, z = 0.f;
  Point3f() {}
  Point3f(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};

// ---- the tracker (src/slam/src/opencv/CvLKStereo.cpp, compiled against this mock by oracle/Makefile into
// oracle/_ref/liblk_reference.so): the names it touches beyond the ones above
template <class T> struct DataType;
template <> struct DataType<unsigned char> { enum { depth = CV_8U }; };
template <> struct DataType<short> { enum { depth = CV_16S }; };
template <> struct DataType<float> { enum { depth = CV_32F }; };

struct TermCriteria {
  enum Type { COUNT = 1, MAX_ITER = COUNT, EPS = 2 };
  int type = 0, maxCount = 0;
  double epsilon = 0.;
  TermCriteria() {}
  TermCriteria(int t, int c, double e) : type(t), maxCount(c), epsilon(e) {}
};

// a buffer of n elements that lives as long as the object and converts to a pointer to its first element
template <class T>
class AutoBuffer {
 public:
  explicit AutoBuffer(size_t n) : v_(n) {}
  operator T*() { return v_.data(); }
  operator const T*() const { return v_.data(); }

 private:
  std::vector<T> v_;
};

}  // namespace cv

// OpenCV's documented meaning, for values an int holds: cvFloor is the largest integer not above the value; cvRound is the
// nearest integer, and a value exactly half way between two integers goes to the even one
inline int cvFloor(double v) { return (int)std::floor(v); }
inline int cvFloor(float v) { return (int)std::floor(v); }
inline int cvRound(double v) {
  const double f = std::floor(v), d = v - f;   // exact: v - floor(v) loses nothing in binary floating point
  const int i = (int)f;
  return d > 0.5 || (d == 0.5 && (i & 1)) ? i + 1 : i;
}
inline int cvRound(float v) { return cvRound((double)v); }

#define CV_Error(code, msg) throw cv::Exception((int)(code), std::string(msg))
#define CV_Assert(expr) do { if (!(expr)) throw cv::Exception((int)cv::Error::StsAssert, std::string(#expr)); } while (0)

#endif
