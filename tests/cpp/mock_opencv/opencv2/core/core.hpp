// tests/cpp/mock_opencv/opencv2/core/core.hpp -- the older spelling of <opencv2/core.hpp>; forwards to the one mock.
#include "../core.hpp"
