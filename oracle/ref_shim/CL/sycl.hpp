// stand-in: <CL/sycl.hpp> is the same header (oracle/ref_shim/README.md)
#pragma once
#include "../sycl/CL/sycl.hpp"
