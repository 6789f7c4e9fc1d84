// Stand-in for mikktspace.h (public struct names only; oracle/ref_shim/README.md): tangents come with the fixtures.
#pragma once
struct SMikkTSpaceContext;
struct SMikkTSpaceInterface {};
struct SMikkTSpaceContext {
    SMikkTSpaceInterface* m_pInterface;
    void* m_pUserData;
};
