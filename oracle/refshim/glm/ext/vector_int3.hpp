// Stand-in for <glm/ext/vector_int3.hpp>: the whole subset lives in one header.
#pragma once
#include "../rt2_glm.hpp"
