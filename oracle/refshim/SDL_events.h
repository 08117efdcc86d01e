// Stub of <SDL_events.h> for the reference build: the fields RayTracer::OnEvent reads.
#pragma once
enum { SDL_WINDOWEVENT_RESIZED = 5 };
struct SDL_WindowEvent {
  unsigned char event;
  int data1, data2;
};
union SDL_Event {
  SDL_WindowEvent window;
};
