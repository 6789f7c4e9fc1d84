// Stand-in for rapidobj (public names only; oracle/ref_shim/README.md): no OBJ file is read.
#pragma once
namespace rapidobj {
struct Result {};
}
