// planes.hip -- the component-plane kernels (kernels/planes.hpp) as a code object of their own; host_planes.inc (in
// somhip.hip) launches them.  Same flags as somhip.hip.
#define SOMHIP_PLANES_DEFINE
#include "kernels/planes.hpp"
