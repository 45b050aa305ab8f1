// TEST INFRASTRUCTURE ONLY.  Part of this project's own stand-in for OpenCV: everything is in opencv2/core/core.hpp.
#include "opencv2/core/core.hpp"
