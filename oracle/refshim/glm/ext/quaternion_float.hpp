// Stand-in for <glm/ext/quaternion_float.hpp>: the whole subset lives in one header.
#pragma once
#include "../rt2_glm.hpp"
