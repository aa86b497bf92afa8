// Kernel instantiations for P256K1 = secp256k1 (see k_weierstrass.inc).  The variable base runs the endomorphism
// ladder by default: the curve has cofactor 1, so sigma(x, y) = (beta x, y) is [lambda] on every point and the signed
// lattice split (kernels_coz.hpp glv_split_lattice) applies to any base.  ECCX_P256K1_GLV=0 builds the plain ladder
// as the default instead (A/B runs).
#define ECCX_CURVE P256K1
#define ECCX_CURVE_U P256K1U
#define ECCX_OPS_NAME ops_P256K1
#define ECCX_GLV_PARAMS P256K1_GLV
#ifndef ECCX_P256K1_GLV
#define ECCX_P256K1_GLV 1
#endif
#define ECCX_EXTRA_OPS(t)                   \
  do {                                      \
    (t).var_glv_default = ECCX_P256K1_GLV;  \
  } while (0)
#define ECCX_ORDER P256K1_ORD
#include "k_weierstrass.inc"
