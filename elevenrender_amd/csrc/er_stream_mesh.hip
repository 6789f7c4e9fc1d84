// er_stream_mesh.hip -- the streaming kernel's instances with the emitter samples of ER_FLAG_MESH_LIGHTS (er_shade.h), in a translation
// unit of their own: er_stream.hip with ER_STREAM_MESH_TU, which compiles its launcher as er_launch_stream_mesh over the MESH = true
// instances only (see the comment above er_probe_stream there).
#define ER_STREAM_MESH_TU
#include "er_stream.hip"
