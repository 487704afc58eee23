// umat.hip -- the U-matrix kernels (kernels/umat.hpp) as a code object of their own; host_umat.inc (in somhip.hip)
// launches them.  Same flags as somhip.hip.
#define SOMHIP_UMAT_DEFINE
#include "kernels/umat.hpp"
