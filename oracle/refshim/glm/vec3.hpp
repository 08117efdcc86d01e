// Stand-in for <glm/vec3.hpp>: the whole subset lives in one header.
#pragma once
#include "rt2_glm.hpp"
