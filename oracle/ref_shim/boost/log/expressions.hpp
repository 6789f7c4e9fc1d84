// stand-in: the build of the reference for tests/golden needs nothing from this header (oracle/ref_shim/README.md)
#pragma once
