// Stub of <imgui.h> for the reference build: the three calls RayTracer::OnImGui names, as no-ops.
#pragma once
namespace ImGui {
inline bool Begin(const char*) { return false; }
inline bool Button(const char*) { return false; }
inline void End() {}
}  // namespace ImGui
