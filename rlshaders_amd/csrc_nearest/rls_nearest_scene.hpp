// rls_nearest_scene.hpp -- what an rls_nearest_scene is: the private layout two libraries share.  librls_nearest.so
// (nearest.hip) makes, queries and frees a scene; librls_nearest_refit.so (refit.hip) borrows one and rewrites its triangle
// records and node boxes in place.  Host code only: no kernel reads this struct, and neither library calls the other.
//
// The struct starts with a layout tag.  rls_nearest_scene_create sets it to kNearestSceneLayout; the refit refuses a scene
// whose tag is not the one it was compiled with, so a refit library beside a nearest library of another layout fails by name
// instead of writing through misread pointers.  Any change to the members below changes the tag.
#ifndef RLS_NEAREST_SCENE_HPP
#define RLS_NEAREST_SCENE_HPP

#include <stddef.h>
#include <stdint.h>

#include "../../include/rlshaders_amd_nearest.h"
#include "rls_nearest_bvh.hpp"

constexpr uint64_t kNearestSceneLayout = 0x524c534e53433032ull;   // "RLSNSC02"

struct rls_nearest_scene {
    uint64_t layout;              // kNearestSceneLayout
    int device;
    void *blob;                   // the one device allocation
    const NearestNode *nodes;
    const NearestTri *tris;
    const uint32_t *index, *surface;
    const float *normals;
    rls_nearest_scene_info info;
    // byte offsets of the blob's parts (nodes, triangle records, vertex indices, surface ids, normals), for a library that
    // writes them: the pointers above are the queries' and const.  A part the scene lacks has its pointer NULL above.
    size_t o_nodes, o_tris, o_index, o_surface, o_normals;
};

#endif
