// Device code of one kernel family for the curve selected with -DMSMZ_CURVE (see instantiate.h).
#include "instantiate.h"
namespace msmz {
#define X(F, Fr) MSMZ_INST_DOT(F, Fr, MSMZ_DEFINE)
MSMZ_WEIERSTRASS_FIELDS(X)
MSMZ_TE_FIELDS(X)
#undef X
}  // namespace msmz
