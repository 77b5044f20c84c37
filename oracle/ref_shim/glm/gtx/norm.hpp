// glm/gtx/norm.hpp -- length2() lives in the stand-in glm.hpp (see there).
#ifndef ORACLE_REF_SHIM_GLM_NORM_HPP
#define ORACLE_REF_SHIM_GLM_NORM_HPP
#include "../glm.hpp"
#endif
