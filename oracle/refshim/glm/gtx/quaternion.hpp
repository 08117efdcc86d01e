// Stand-in for <glm/gtx/quaternion.hpp>: the whole subset lives in one header.
#pragma once
#include "../rt2_glm.hpp"
