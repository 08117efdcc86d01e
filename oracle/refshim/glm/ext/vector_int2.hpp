// Stand-in for <glm/ext/vector_int2.hpp>: the whole subset lives in one header.
#pragma once
#include "../rt2_glm.hpp"
