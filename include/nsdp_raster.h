/*
 * nsdp_raster.h -- packed triangle meshes rasterised into depth, face and weight images, libnsdp_hip.so (ABI version 30): for
 * every pixel of every image the nearest face that covers the pixel's centre (its depth, the face and, optionally, the
 * perspective-correct barycentric weights) and, optionally, the number of faces that cover it.  nsdp_amd/rasterize.py wraps it
 * (Camera, RasterPlan, rasterize, interpolate, shade).
 *
 * The conventions are those of nsdp_raycast.h: device pointers + sizes, dense row-major tensors, outputs and the workspace
 * allocated by the caller and possibly UNINITIALISED on entry, `stream` a hipStream_t passed as void*, 0 / negative NSDP_E* /
 * positive hipError_t as the return value, the message in nsdp_last_error().  Sizes are judged before the flags, the flags before
 * pointers and pointers before anything is launched.  The packed layout: rows(cap,3) + offsets(B+1) i32 on the device for the
 * vertices and the faces, the vertex indices of a face LOCAL to its mesh; every offsets entry is clamped to [previous entry,
 * cap] as the kernels read it, every vertex index is clamped into its mesh's range before it forms an address and every entry
 * of image_shape is clamped into 0 .. B-1, so a stale tensor gives wrong numbers and never an access outside the operands.  The
 * host reads no device memory: the grids are sized from I, H, W and the capacities, and a captured launch is valid for any
 * offsets.  Only the bytes declared here are touched; every byte of the workspace that is read was written by the same call.
 * No atomics: two runs give the same bits.  Every element of every output is written exactly once.
 *
 * Limits: 1 <= H, W <= 4096, 1 <= I <= 65535, I * H * W < 2^31, and nsdp_mesh_ray_cast's limits on the meshes: 1 <= B <= 65535,
 * vcap and fcap in 1 .. 1 048 576 * B.  Flags other than bit 0 are refused.
 *
 * tests/raster_ref.py is the rule below in numpy, operation by operation; tests/test_raster_arena_gpu.py holds the launching
 * entry inside the poisoned arena; tools/raster_host_check.cpp runs the bad-argument table on the host.
 */
#ifndef NSDP_RASTER_H_
#define NSDP_RASTER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* flags of nsdp_mesh_rasterize */
#define NSDP_RASTER_FRONT_ONLY 1 /* bit 0: only faces whose three edge signs are all +1 cover a pixel */

/* Bytes of workspace of nsdp_mesh_rasterize: per image and per block of 64 faces -- fcap / 64 + B + 1 blocks, a mesh's blocks
 * start at its first face, as in nsdp_raycast.h -- a screen box of four i32 and one i32 count of dropped faces:
 * 20 * I * (fcap / 64 + B + 1).  0 for sizes the entry refuses.  Host only. */
size_t nsdp_mesh_rasterize_workspace_bytes(int B, int I, int fcap);

/* verts(vcap,3) f32 + vert_offsets(B+1), faces(fcap,3) i32 + face_offsets(B+1), cams(I,16) f32: per image a row-major 4 x 4
 * matrix M with rows X, Y, Z, W, image_shape(I) i32: the mesh image i looks at (clamped into 0 .. B-1; a mesh may have any
 * number of views)  ->  depth_out(I,H,W) f32 (FLT_MAX where nothing covers the pixel), face_out(I,H,W) i32 (a PACKED face row,
 * -1 where empty), bary_out(I,H,W,3) f32 or NULL (0 where empty), count_out(I,H,W) i32 or NULL, dropped_out(I) i32.
 *
 * THE RULE.  fp32, int64 and fp64 as named, every floating-point operation rounds once, no contraction.
 *
 *   Corner (fp32).  For a vertex (x, y, z) and the image's M:  X = ((M00 * x + M01 * y) + M02 * z) + M03, and likewise Y, Z, W
 *   from rows 1, 2, 3.  A function of the vertex and the camera alone: faces that share a vertex see the same corner.
 *   px = X / W, py = Y / W (correctly rounded divisions), in pixel units: the centre of pixel (row j, column i) is
 *   (i + 1/2, j + 1/2).
 *
 *   Snap.  sx = rint(px * 256), sy = rint(py * 256) (the product in fp32, rint to the nearest integer, ties to even), taken as
 *   integers.  Pixel centres are the integers (256 i + 128, 256 j + 128).
 *
 *   Dropped.  A corner is good where W > 0, X, Y, Z and W are finite and |rint(px * 256)| <= 2^24 and |rint(py * 256)| <= 2^24
 *   (compared in fp32, so an overflowed quotient is not good).  A face with a corner that is not good is DROPPED: it covers
 *   nothing and is counted in dropped_out of every image of its mesh.  THERE IS NO NEAR-PLANE CLIPPING: a mesh that passes
 *   through the camera plane W = 0 loses the faces that reach it, whole.
 *
 *   Edge sign (exact, int64).  With c the pixel centre and P' = P - c, Q' = Q - c on the snapped integers, for the ORDERED pair
 *   (P, Q):  E = Q'x * P'y - Q'y * P'x,  s = sign(E); where E = 0, s = sign(Qy - Py); where that is 0, s = sign(Px - Qx);
 *   otherwise 0.  Coordinates are at most 2^24 and centres below 2^21, so differences are below 2^25 and E below 2^51: nothing
 *   overflows.  This is nsdp_raycast.h's edge sign: the sign of the edge function at the centre displaced symbolically by
 *   (e, e^2), e > 0 small.  E is linear in c with the gradient (Qy - Py, Px - Qx) -- the two tie-breakers are its components.
 *
 *   Covered.  Face (a, b, c), not dropped, covers the pixel where s(b, c), s(c, a), s(a, b) are all +1 or all -1 (both
 *   orientations count); with NSDP_RASTER_FRONT_ONLY only where all are +1 -- on a screen whose rows run downwards (py grows
 *   down the image) those are the faces whose corners run counter-clockwise as the viewer sees them.  A face of zero snapped
 *   area is never covered (a generic point is strictly inside no segment) and is not counted as dropped.
 *
 *   Depth and weights (fp64), perspective-correct, for a covering face:  ea = |E(b, c)|, eb = |E(c, a)|, ec = |E(a, b)| (exact
 *   as doubles),  iwa = 1.0 / double(Wa) and likewise iwb, iwc,  ta = ea * iwa, tb = eb * iwb, tc = ec * iwc,
 *   s = (ta + tb) + tc,  bary = fp32(ta / s), fp32(tb / s), fp32(tc / s) (the weights of a, b, c),
 *   depth = fp32(((ta * Za + tb * Zb) + tc * Zc) / s) with Z the corner's fp32 third row widened to double.  All W > 0 and
 *   the e's are magnitudes, not all zero on a covering face (the argument of nsdp_raycast.h), so s > 0 and nothing cancels.
 *
 *   Result.  The pixel keeps the minimum of the 64-bit keys (ordered(depth) << 32 | packed face row) over the covering faces and
 *   the start key (FLT_MAX, no face = 0xFFFFFFFF), where ordered(d) maps the fp32 bits u of d to ~u where the sign bit is set
 *   and to u | 0x80000000 otherwise (an order-preserving map of the floats to unsigned integers; -0 sorts below +0).  The
 *   smallest face row wins among equal depth bits, whatever the order of the visit.  depth_out holds the winner's depth,
 *   bary_out its weights by the operations above, count_out the number of covering faces (with NSDP_RASTER_FRONT_ONLY: of
 *   those the flag keeps).
 *
 * WHAT FOLLOWS.  Coverage is the EXACT coverage of the snapped corners by a generic point: no rounding enters a sign.  So a
 * closed mesh (every edge used by two faces) none of whose faces is dropped covers every pixel an even number of times, and a
 * pixel centre on a shared edge or vertex is never counted twice by same-facing neighbours, nor missed by both.
 * The envelope of depth against the exact rational value d* on the same snapped corners and fp32 X, Y, Z, W:
 *   |depth - d*| <= 2^-24 |d*| + 11 * 2^-53 max(|Za|, |Zb|, |Zc|)
 *       (iw one fp64 rounding, t one more; every term of the numerator carries those two, its product's and at most two sums':
 *       5; every term of s the two and at most two sums': 4; the quotient 1: ten roundings of 2^-53 on terms that do not
 *       cancel in s and are at most s max|Z| in the numerator -- the eleventh covers every second-order term; then one fp32
 *       rounding.)
 *
 * THE KERNELS.  raster_boxes: one wave per block of 64 consecutive faces of the image's mesh -- the box of the snapped corners
 * of its faces that are not dropped, and the number that are, into the workspace.  raster_tiles: one workgroup of 256 lanes per
 * tile of 16 x 16 pixels and image, one pixel per lane -- the lanes read 256 block boxes at a time and keep the blocks that
 * touch the tile; each of the four waves recomputes one such block's corners, keeps the faces whose own box touches the tile and
 * stages their edge functions at the tile's first centre in LDS; every lane tests every staged face (two fp64 products and two
 * sums per edge, exact: all values are integers below 2^53); the best key and the count live in registers and the lane writes
 * its pixel once.  raster_dropped: one wave per image sums the blocks' counts in a fixed order.
 *
 * workspace: 16-byte aligned, nsdp_mesh_rasterize_workspace_bytes(B, I, fcap) bytes. */
int nsdp_mesh_rasterize(const float *verts, const int32_t *vert_offsets, const int32_t *faces, const int32_t *face_offsets,
                        const float *cams, const int32_t *image_shape, int B, int I, int vcap, int fcap, int H, int W, int flags,
                        void *workspace, float *depth_out, int32_t *face_out, float *bary_out, int32_t *count_out,
                        int32_t *dropped_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSDP_RASTER_H_ */
