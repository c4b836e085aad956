/* dlpd.h -- C ABI of libdlpd.so: MI355X (gfx950) kernels for the exhaustive rotation x translation
 * correlation search of DeepLocalProteinDocking.
 *
 * The reference has no FFI; its boundary for this path is Python duck typing onto
 * TorchProteinLibrary operator objects.  Each entry point below names the
 * reference call site (file:line under /root/reference) whose arithmetic it replaces.  All
 * functions: plain pointers and sizes, device pointers are borrowed for the duration of the call,
 * work is enqueued on `stream` (a hipStream_t passed as void*), no allocation, no host
 * synchronisation, return 0 on success (DLPD_ERR_* otherwise), never throw.
 *
 * Layouts: volumes are (.., L, L, L) float32, index [x][y][z], z contiguous.  N = 2L,
 * NZ = N/2 + 1.  Spectra are (.., NZ, N, N) complex64 indexed [kz][kx][ky].
 *
 * THE PATH -- the minimal call set of one search (Docker.py:184-238; what DockingEngine issues in steady state):
 *   once per pair    dlpd_rfft3d_padded        receptor spectrum            (DockingModels.py:71, hoisted out of the loop)
 *                    dlpd_receptor_pack        ... in K2's read order       (boxes 80 / 40 only)
 *                    dlpd_receptor_order       ... in K2's fetch order      (boxes 64 / 32 only)
 *                    dlpd_make_channels_last   ligand copy K1 gathers from
 *   per launch       dlpd_zfft_channels_last   K1: rotation + z transform  (Docker.py:218)
 *                    dlpd_project_atoms + dlpd_zfft_into   clash channel from rotated atoms (Docker.py:221-224)
 *                    dlpd_xy_correlate_packed / dlpd_xy_correlate   K2     (DockingModels.py:70-71, Docker.py:225)
 *                    dlpd_zifft_filter_cand    K3: z inverse + clip + MLP + clash mask + candidates (DockingModels.py:74-83, Docker.py:226-232)
 *                    dlpd_topk_select_cand, dlpd_topk_merge_tau   the ranked list (Docker.py:86-105)
 *   two resolutions  the same K1 / K2 on the coarse grid, then dlpd_zifft_preact (coarse) and dlpd_zifft_filter_cand(aux = its planes)
 * Everything else in this header is a VARIANT of one of these stages -- suffix _ext (embedded box), _oriented / _quads (launch
 * variants of the per-channel K1), _form (kernel formulation named: test cross-checks), _occ (occupancy maps: sparse ligands),
 * _aux / un-suffixed (fewer features) -- a stand-alone operator of the plugin surface (dlpd_rotate_trilinear,
 * dlpd_correlate_generic, dlpd_local_*, dlpd_filter_*, dlpd_conv3d*, dlpd_maxpool3d_5s2*), or a size / capability query.  Test hooks
 * (dlpd_debug_*) are declared in dlpd_debug.h, not here.
 */
#ifndef DLPD_H
#define DLPD_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DLPD_OK 0
#define DLPD_ERR_ARG 1
#define DLPD_ERR_UNSUPPORTED 2
#define DLPD_ERR_LAUNCH 3

int dlpd_version(void);
/* sha256 (64 hex digits) of the sources, headers and flags this library was built from; the build
 * script refuses a library whose hash differs from the sources next to it */
const char* dlpd_source_hash(void);
/* 1 if box size L has a compiled pipeline: L in {32, 40, 64, 80} (grids N = 2L = 64, 80, 128, 160) */
int dlpd_grid_supported(int L);
/* 1 if dlpd_xy_correlate_oriented(transposed = 1) exists for box L (slabs the per-channel K1 stored transposed): every
 * compiled box except 80, whose transposed reader is a test variant (-DDLPD_TEST_VARIANTS), not part of libdlpd.so. */
int dlpd_orientation_supported(int L);
/* hidden width the filter kernel pads H to (2,4,8,16,24,32), -1 if H > 32 */
int dlpd_hidden_pad(int H);
/* Hidden width the FUSED pipeline (dlpd_zifft_filter*, dlpd_zifft_preact) pads H to on a fine grid of L^3 voxels
 * (two_res: with a coarse (L/2)^3 grid, ProteinRepresentationModels.py:72-76): dlpd_hidden_pad's widths plus 48 -- the
 * reference class default SimpleFilter([32, 64]) has hidden width 48 (DockingModels.py:25-27) -- where the role-split
 * K3 is compiled (L = 64, 80; coarse 40); -1: no fused kernel for this width, use dlpd_filter_mask. */
int dlpd_fused_hidden_pad(int H, int L, int two_res);

/* TPL VolumeRotation call, src/Docker/Docker.py:218 (ctor :40; DockingModels.py:49).
 * out[b,c](i) = trilinear vol[b,c]( center + R_b^T (i - center) ), zeros outside.
 * R_b is used as a GENERAL 3x3 map by every rotation entry point of this header (nothing assumes orthonormality): a
 * sampling scale s and a reversed axis order (matrix axis 0 <-> last spatial index) -- conventions TorchProteinLibrary's
 * VolumeRotation may have (its source is absent) -- are passed as R' = s P R P, P the axis reversal
 * (deeplocalproteindocking_amd/Utils/Conventions.py: kernel_matrices), the pivot as `center`.
 * vol (B,C,L^3) with batch stride vol_bstride floats (0: one volume set shared by all b). */
int dlpd_rotate_trilinear(const float* vol, const float* R, float* out, int B, int C, int L,
                          long long vol_bstride, float center, void* stream);
/* The adjoint of that call (TPL's VolumeRotation is a differentiable operator; src/Docker/Docker.py:218 is the call a model
 * trained on a search's top list differentiates): gout (B,C,L^3) the gradient of `out`, R and center as the forward took them,
 *   gvol[b,c](q) = sum_i w_b(i, q) gout[b,c](i),  w_b(i, q) the trilinear weight the forward's sample of output voxel i gives
 *   source voxel q (corners outside the box carry none).
 * gvol is laid out as vol was: (B,C,L^3) with batch stride gvol_bstride floats, or, for stride 0 (one volume set shared by all
 * b), (C,L^3) = the sum over b, added in the order of b.  accumulate != 0: the sums start at the values gvol holds (B split
 * over several calls gives the bits of one call) instead of 0.  A gather over the output voxels that can reach q -- exact for
 * any invertible 3x3 map --: no atomics, no workspace, every element written once, the same bits run to run.
 * Null pointers, B or C <= 0 or a negative stride: DLPD_ERR_ARG; L < 2 or L > 128: DLPD_ERR_UNSUPPORTED. */
int dlpd_rotate_trilinear_grad(const float* gout, const float* R, float* gvol, int B, int C, int L, long long gvol_bstride,
                               float center, int accumulate, void* stream);
/* The gradient of that call with respect to the MATRICES (what a descent of a docking score in the pose itself needs):
 *   gR[b][3j + a] = sum_c sum_i gout[b,c](i) * d_a vol[b,c]( p_b(i) ) * (i_j - center),
 *   p_a(i) = center + sum_j R[b][3j + a] (i_j - center) the forward's sample position, d_a the derivative of the trilinear
 *   sample along axis a: the same floor, in-box masks and corners as the forward (on a cell face: the right-hand derivative).
 * gout (B,C,L^3); vol, R, vol_bstride and center as the forward took them; gR (B,9) laid out as R, every element written.
 * Per voxel the sum over the channels is a float32 chain, everything after it float64: block partials go to ws
 * (dlpd_rotate_trilinear_rgrad_ws_bytes(B, L) bytes; 0 for an unsupported shape) and are added in block order -- no atomics,
 * the same bits run to run, and a pose's nine numbers do not depend on the other poses of its call.
 * Null pointers, B or C <= 0 or a negative stride: DLPD_ERR_ARG; L < 2 or L > 128: DLPD_ERR_UNSUPPORTED. */
size_t dlpd_rotate_trilinear_rgrad_ws_bytes(int B, int L);
int dlpd_rotate_trilinear_rgrad(const float* gout, const float* vol, const float* R, float* gR, void* ws, int B, int C, int L,
                                long long vol_bstride, float center, void* stream);
/* SUB-VOXEL TRANSLATIONS: the same rotation with a per-pose offset of the sample position,
 *   p_a(i) = (center + off[b][a]) + sum_j R[b][3j + a] (i_j - center),   off (B,3) float32 in voxels of the source volume, laid
 *   out like a row of R's columns; null: zeros.  center + off is added first, the rotated term then: with off = 0 (or null) every
 *   entry returns the bits of the plain entry.  A volume rotated and then displaced by s voxels is off = -R^T s.
 * dlpd_rotate_trilinear_shift: the forward (vol, R, out, vol_bstride as dlpd_rotate_trilinear; every element written).
 * dlpd_rotate_trilinear_shift_grad: its adjoint with respect to the volume -- dlpd_rotate_trilinear_grad with the offset (the
 *   candidates of a source voxel q are centred on center + A^-1 (q - center - off)); the same guarantees: no atomics, every
 *   element written, accumulate, exact for any invertible map.
 * dlpd_rotate_trilinear_pgrad: the pose gradient -- gR (B,9) as dlpd_rotate_trilinear_rgrad, and
 *   goff[b][a] = sum_c sum_i gout[b,c](i) * d_a vol[b,c]( p_b(i) )   (B,3); either may be null (not wanted), not both.
 *   The same order of additions as the nine-number entry (its gR at off = 0 has that entry's bits); twelve float64 partials per
 *   block in ws (dlpd_rotate_trilinear_pgrad_ws_bytes(B, L) bytes; 0 for an unsupported shape), added in block order; a pose's
 *   twelve numbers do not depend on the other poses of its call.
 * Null pointers, B or C <= 0 or a negative stride: DLPD_ERR_ARG; L < 2 or L > 128: DLPD_ERR_UNSUPPORTED. */
int dlpd_rotate_trilinear_shift(const float* vol, const float* R, const float* off, float* out, int B, int C, int L,
                                long long vol_bstride, float center, void* stream);
int dlpd_rotate_trilinear_shift_grad(const float* gout, const float* R, const float* off, float* gvol, int B, int C, int L,
                                     long long gvol_bstride, float center, int accumulate, void* stream);
size_t dlpd_rotate_trilinear_pgrad_ws_bytes(int B, int L);
int dlpd_rotate_trilinear_pgrad(const float* gout, const float* vol, const float* R, const float* off, float* gR, float* goff,
                                void* ws, int B, int C, int L, long long vol_bstride, float center, void* stream);

/* Stage K1 of TPL VolumeConvolution (src/Models/DockingModels.py:71, src/Docker/Docker.py:225),
 * optionally fused with the rotation of Docker.py:218: z-axis R2C of (rotated) volumes.
 * wsA: nb*CT*NZ*L*L complex64. */
int dlpd_zfft(const float* vol, const float* R, void* wsA, int nb, int CT, int L, long long vol_bstride,
              int do_rotate, float center, void* stream);

/* Same, writing channels [c_base, c_base+CT) of a (nb, CT_out, NZ, L, L) workspace: lets the clash
 * channel come from per-rotation re-projected atoms (Docker.py:221-224) while the score channels are
 * rotated volumes (Docker.py:218). */
int dlpd_zfft_into(const float* vol, const float* R, void* wsA, int nb, int CT, int CT_out, int c_base, int L,
                   long long vol_bstride, int do_rotate, float center, void* stream);
/* dlpd_zfft_into for GIVEN volumes (no rotation; Docker.dockE3's per-batch representation, Docker.py:163-172) that come with
 * occupancy maps: occ (nb, ceil(L/4)^3) bytes, one map per batch entry for all its CT channels, non-zero where the 4 x 4 x 4
 * cell holds a non-zero value (the maps dlpd_conv3d_split_sparse / dlpd_maxpool3d_5s2_sparse hand on).  Voxels of empty
 * cells are taken as zero and NOT read (unwritten activations), x-planes without an occupied cell are written as zeros
 * without a transform -- or, with skip_empty != 0, not written at all: for a consumer that goes by the pencil map (the maps'
 * OR over z; dlpd_xy_correlate_packed_occ).  Same spectra as dlpd_zfft_into on the dense tensor. */
int dlpd_zfft_volumes_occ(const float* vol, const unsigned char* occ, void* wsA, int nb, int CT, int CT_out, int c_base, int L,
                          long long vol_bstride, int skip_empty, void* stream);

/* Slab orientation (speed only, results identical).  With transposed = 1 every rotation of the call is
 * processed with the roles of x and y exchanged and its slabs are stored as [kz][y][x]: the caller groups the
 * rotations whose sample matrix has |R[0][2]| > |R[1][2]| (source z axis closer to the output x axis) into such
 * calls, so that the gather of Docker.py:218 runs along contiguous memory for them as well.  Channels written
 * by separate calls (e.g. the re-projected clash volume) must use the same value.
 * dlpd_xy_correlate_oriented undoes the transposition while it stages each slab. */
int dlpd_zfft_oriented(const float* vol, const float* R, void* wsA, int nb, int CT, int CT_out, int c_base, int L,
                       long long vol_bstride, int do_rotate, float center, int transposed, void* stream);
int dlpd_xy_correlate_oriented(const void* wsA, const void* rec, void* wsB, int nb, int CT, int L,
                               long long rec_bstride, int transposed, void* stream);

/* Quad layout of a volume set for the rotation gather: quads[v][x][y][z] (y, z < L-1) = {vol(x,y,z), vol(x,y,z+1),
 * vol(x,y+1,z), vol(x,y+1,z+1)}: the eight trilinear corners are two 16-byte gathers instead of four 8-byte
 * ones (the gather is bound by cache lines touched per instruction).  dlpd_zfft_quads = dlpd_zfft_oriented with
 * do_rotate = 1 on one volume set shared by all rotations; results are bit-identical to the plain path. */
size_t dlpd_quads_floats(int nvol, int L);
int dlpd_make_quads(const float* vol, float* quads, int nvol, int L, void* stream);
int dlpd_zfft_quads(const float* quads, const float* R, void* wsA, int nb, int CT, int CT_out, int c_base, int L,
                    float center, int transposed, void* stream);

/* Channels-last copy of a ligand's C score volumes for the rotation gather of Docker.py:218: cl[x][y][z][Cp], Cp = C
 * rounded up to 16 (zero padded).  Every channel is sampled at the same rotated position, so one 16-byte load
 * serves four channels of a corner and the gather's cache-line requests per sample stop depending on the rotation
 * (no slab orientation, no quad layout on this path).  dlpd_zfft_channels_last = dlpd_zfft_into with do_rotate = 1
 * for channels [c_base, c_base + C) of a (nb, CT_out, NZ, L, L) workspace; samples are bit-identical to the plain
 * path.  A clash channel is written by a separate dlpd_zfft_into call (transposed = 0). */
size_t dlpd_channels_last_floats(int C, int L);
int dlpd_make_channels_last(const float* vol, float* cl, int C, int L, void* stream);
int dlpd_zfft_channels_last(const float* cl, const float* R, void* wsA, int nb, int C, int CT_out, int c_base, int L,
                            float center, void* stream);

/* The same two rotation + z-transform entries for a volume that is an extent^3 box in the corner of the L^3 one (zeros
 * around it): a box_size without a compiled plan inside the next compiled box (box_size is a free argument of
 * Docker.py:18; Docker._dock_volumes_embedded).  `center` is the pivot of the SMALL box; output voxels with any index
 * >= extent are written as zero -- the reference crops the rotated volume to its own box (Docker.py:218).
 * extent = 0 or L: the plain entries above. */
int dlpd_zfft_oriented_ext(const float* vol, const float* R, void* wsA, int nb, int CT, int CT_out, int c_base, int L,
                           long long vol_bstride, int do_rotate, float center, int transposed, int extent, void* stream);
int dlpd_zfft_channels_last_ext(const float* cl, const float* R, void* wsA, int nb, int C, int CT_out, int c_base, int L,
                                float center, int extent, void* stream);
/* ... with the kernel formulation named: 0 = the library's default, 1 = every wave gathers, transforms and stores in turn
 * (k_rotate_zfft_cl), 2 = gather waves and transform / store waves with fixed roles, one block per CU walking a range of
 * work items (k_rotate_zfft_cl_rs).  Same samples, same butterflies: the spectra are bit-identical.  Form 2 is a TEST VARIANT:
 * it exists in -DDLPD_TEST_VARIANTS builds only (tests/variants/libdlpd_variants.so, boxes 64 and 80); libdlpd.so returns
 * DLPD_ERR_UNSUPPORTED for it at every box -- dlpd_k1_form_supported(L, form) says what the loaded library holds. */
int dlpd_k1_form_supported(int L, int form);
int dlpd_zfft_channels_last_form(const float* cl, const float* R, void* wsA, int nb, int C, int CT_out, int c_base, int L,
                                 float center, int extent, int form, void* stream);
/* The same gather with per-rotation OCCUPANCY MAPS (round 6; Docker.py:218 for a ligand whose representation is zero away
 * from the protein -- any real one).  dlpd_rotated_occupancy turns the stored ligand's cell map (occ_src, ceil(L/4)^3 bytes,
 * dlpd_conv3d_tile_occupancy over all its channels) into one conservative map per rotation (occ_out, nb maps: 0 = every
 * trilinear sample of that 4 x 4 x 4 cell of the rotated volume is certainly zero); R are the matrices K1 samples with.
 * dlpd_zfft_channels_last_occ is dlpd_zfft_channels_last_ext that skips the loads of samples in empty cells and the
 * transform of blocks without an occupied cell (their zeros are written).  Same spectra.
 * pencil_out (may be null; nb x ceil(L/4) 32-bit words, [rotation][x cell]): bit (y cell) set where some z cell of that column
 * is marked; dlpd_pencil_bits makes the same words from nb given cell maps (the plugin's own, dlpd_zfft_volumes_occ).
 * skip_empty != 0: blocks without an occupied cell write NOTHING -- for a consumer that goes by the pencil map and never reads
 * those pencils: dlpd_xy_correlate_packed_occ (boxes with a packed receptor: dlpd_pencil_map_supported(L)), which takes the
 * pencils the map marks empty as zeros for channels [0, nmasked) (the clash channel behind them is read as it is). */
int dlpd_rotated_occupancy(const unsigned char* occ_src, const float* R, unsigned char* occ_out, unsigned* pencil_out, int nb,
                           int L, float center, void* stream);
int dlpd_pencil_bits(const unsigned char* occ, unsigned* pencil_out, int nb, int L, void* stream);
int dlpd_zfft_channels_last_occ(const float* cl, const float* R, const unsigned char* occ, void* wsA, int nb, int C, int CT_out,
                                int c_base, int L, float center, int extent, int skip_empty, void* stream);
int dlpd_pencil_map_supported(int L);
int dlpd_xy_correlate_packed_occ(const void* wsA, const void* rec_packed, void* wsB, int nb, int CT, int L,
                                 const unsigned* pencil_map, int nmasked, void* stream);
/* CHUNK-MAJOR copy of the same C score volumes: buf[chunk][x][y][z][CC], CC = the channels one K1 block transforms at that
 * box (8 at box 64, 16 at the others), channels zero padded to whole chunks -- never larger than the channels-last copy.
 * A K1 block gathers CC channels of each corner; in cl[x][y][z][Cp] those are a CC-channel slice of every voxel's record (at
 * 48 channels and box 64: 32 of every 128-byte line it pulls into its L1), here the CC channels of neighbouring z are
 * adjacent and the block uses every line it fetches whole.  dlpd_zfft_channel_chunks is dlpd_zfft_channels_last_ext (occ
 * null) / dlpd_zfft_channels_last_occ (occ given; skip_empty as there) reading this copy: only addresses differ, the spectra
 * are bit-identical.  dlpd_channel_chunks_default(L): 1 where the engine gathers from this copy unless told otherwise. */
size_t dlpd_channel_chunks_floats(int C, int L);
int dlpd_channel_chunks_default(int L);
int dlpd_make_channel_chunks(const float* vol, float* buf, int C, int L, void* stream);
int dlpd_zfft_channel_chunks(const float* buf, const float* R, const unsigned char* occ, void* wsA, int nb, int C, int CT_out,
                             int c_base, int L, float center, int extent, int skip_empty, void* stream);

/* CoordsRotate + CoordsTranslate + TypedCoords2Volume (+ channel sum) of src/Docker/Docker.py:204,
 * 208,221-224 in one kernel: p' = R_b p + shift, density exp(-|r - p'|^2 / 2) on the 5^3 voxels
 * around each atom (build-defined shape).  coords (B, 3*stride_atoms) ordered by type,
 * num_atoms_of_type / offsets (B, ntypes) int32.  out (B, ntypes, L^3) or (B, 1, L^3) if sum_types. */
int dlpd_project_atoms(const float* coords, const int* num_atoms_of_type, const int* offsets, const float* R,
                       float shift_x, float shift_y, float shift_z, float* out, int B, int stride_atoms,
                       int ntypes, int L, float resolution, int sum_types, void* stream);
/* The same with the density shape as parameters (TypedCoords2Volume's is not known: TorchProteinLibrary is absent from
 * the reference tree; scripts/calibrate_tpl.py determines them where it is installed): exp(-|r - p'|^2 / (2 sigma^2)) on
 * the (2 window + 1)^3 voxels around each atom, times `norm` (0 < norm <= 64; the fixed-point accumulator holds
 * 1023 per voxel), voxel (i,j,k) at ((i,j,k) + voxel_offset) * resolution; window <= 6.
 * dlpd_project_atoms = (sigma 1, window 2, voxel_offset 0, norm 1). */
int dlpd_project_atoms_ext(const float* coords, const int* num_atoms_of_type, const int* offsets, const float* R,
                           float shift_x, float shift_y, float shift_z, float* out, int B, int stride_atoms,
                           int ntypes, int L, float resolution, int sum_types, float sigma, int window,
                           float voxel_offset, float norm, void* stream);
/* The same projection (all types, no sum) CELL-WISE, for consumers that go by occupancy maps (Docker.dockE3's per-batch
 * projection, Docker.py:163-165, in front of dlpd_conv3d_split_sparse(unwritten != 0)): only the 4 x 4 x 4 cells an atom's
 * window reaches are cleared, accumulated into and converted; occ (B, ceil(L/4)^3 bytes, written in full) marks them; out
 * (B, ntypes, L^3) holds the same values as dlpd_project_atoms_ext in marked cells and is NOT WRITTEN elsewhere. */
int dlpd_project_atoms_cells(const float* coords, const int* num_atoms_of_type, const int* offsets, const float* R,
                             float shift_x, float shift_y, float shift_z, float* out, unsigned char* occ, int B, int stride_atoms,
                             int ntypes, int L, float resolution, float sigma, int window, float voxel_offset, float norm,
                             void* stream);

/* Zero-padded 3-D R2C spectrum (receptor side of VolumeConvolution, DockingModels.py:71):
 * spec (nvol, NZ, N, N) = scale * rfftn(pad(vol)).  wsA: nvol*NZ*L*L complex64 scratch. */
int dlpd_rfft3d_padded(const float* vol, void* spec, void* wsA, int nvol, int L, float scale, void* stream);

/* Stage K2: per (b,c,kz) slab 2-D FFT, multiply rec * conj(lig), 2-D inverse.
 * rec (CT spectra, or nb*CT with rec_bstride = CT*NZ*N*N); wsB: nb*CT*NZ*N*N complex64. */
int dlpd_xy_correlate(const void* wsA, const void* rec, void* wsB, int nb, int CT, int L,
                      long long rec_bstride, void* stream);

/* The same stage for ONE receptor shared by the whole batch (the search: Docker.py:213-232 scores every rotation of the
 * ligand against the same receptor) on the boxes whose K2 re-reads the receptor spectrum for every rotation (80 and 40:
 * their slab does not stay in registers): dlpd_receptor_pack re-orders the spectrum ONCE into the order K2's column
 * phase consumes it (contiguous kilobytes per instruction instead of 64- / 32-byte runs), dlpd_xy_correlate_packed reads
 * that copy.  Same arithmetic, same results bit for bit.  dlpd_receptor_packed_floats: floats of the packed copy (as
 * many as the spectrum), 0 for boxes that take the natural layout only. */
long long dlpd_receptor_packed_floats(int CT, int L);
int dlpd_receptor_pack(const void* rec, void* packed, int CT, int L, void* stream);
int dlpd_xy_correlate_packed(const void* wsA, const void* rec_packed, void* wsB, int nb, int CT, int L, void* stream);

/* The same for boxes 64 and 32, whose K2 keeps a rotation's receptor values in registers and fetches one column set's
 * worth per rotation: dlpd_receptor_order copies the spectrum ONCE into the order of those fetches ([slab][column set]
 * [instruction][lane]: 512 contiguous bytes per instruction from one base address instead of eight 64-byte runs at
 * computed addresses), dlpd_xy_correlate_ordered reads that copy (untransposed slabs, one receptor for the batch).  Same
 * arithmetic, same results bit for bit.  dlpd_receptor_ordered_floats: floats of the copy (as many as the spectrum), 0
 * for every other box. */
long long dlpd_receptor_ordered_floats(int CT, int L);
int dlpd_receptor_order(const void* rec, void* ordered, int CT, int L, void* stream);
int dlpd_xy_correlate_ordered(const void* wsA, const void* rec_ordered, void* wsB, int nb, int CT, int L, void* stream);

/* VolumeConvolution (Docker.py:32,225; DockingModels.py:48,71) for ANY box size -- `box_size` is a free constructor
 * argument of the reference's Docker (Docker.py:18,22-24,31): out (nvol, N^3)[t mod N] = sum_r v1[r + t] v2[r], N = 2L,
 * optional clamp to +-clip.  Direct O(n N) transforms, no radix plan: the slow path for boxes without a compiled
 * pipeline (dlpd_grid_supported(L) == 0), L <= 128.  ws: dlpd_correlate_generic_ws_bytes(nvol, L) bytes of scratch. */
int dlpd_generic_box_supported(int L);
size_t dlpd_correlate_generic_ws_bytes(int nvol, int L);
int dlpd_correlate_generic(const float* v1, const float* v2, float* out, int nvol, int L, int has_clip, float clip,
                           void* ws, void* stream);

/* The BACKWARD of VolumeConvolution (the reference trains GlobalDockingModel through it: DockingModels.py:48,71) for an
 * incoming gradient gout (nvol, N^3) over the whole grid:
 *   g1[s] = sum_r gout[(s - r) mod N] v2[r],  g2[r] = sum_s gout[(s - r) mod N] v1[s],  both (nvol, L^3), s, r in [0, L)^3.
 * Compiled boxes (dlpd_correlate_grad_supported(L): the boxes of dlpd_grid_supported): spec1, spec2 (nvol, NZ, N, N) are
 * dlpd_rfft3d_padded(scale = 1) of v1, v2; ws: dlpd_correlate_grad_ws_bytes(nvol, L) bytes of scratch.  A null g1 / g2 skips
 * that gradient, and the spectrum only it reads (spec2 for g1, spec1 for g2) may then be null too.  No atomics: the same
 * bits on every run. */
int dlpd_correlate_grad_supported(int L);
size_t dlpd_correlate_grad_ws_bytes(int nvol, int L);
int dlpd_correlate_grad(const float* gout, const void* spec1, const void* spec2, float* g1, float* g2, void* ws, int nvol,
                        int L, void* stream);
/* ... and of dlpd_correlate_generic (DockingModels.py:48,71 on a box without a compiled plan, Docker.py:18): the same
 * gradients from the volumes themselves, by the direct transforms, L <= 128.  ws: dlpd_correlate_generic_grad_ws_bytes. */
size_t dlpd_correlate_generic_grad_ws_bytes(int nvol, int L);
int dlpd_correlate_generic_grad(const float* gout, const float* v1, const float* v2, float* g1, float* g2, int nvol, int L,
                                void* ws, void* stream);

/* LOCAL DOCKING -- MultiplyVolumes (src/Models/MultiplyVolumes.py:13-60) under a rotation, LocalDockingModel.forward
 * (src/Models/DockingModels.py:102-120; caller LocalTrainer.score, src/Training/LocalTrainer.py:146-177): the per-channel
 * correlation of the receptor with a ligand under an ARBITRARY rotation at a HANDFUL of translations, by direct summation.
 *   corr (P, C, W^3)[p,c,d] = sum_x rec[c, x + tau] lig'[c, x],  W = 2r + 1, d in [-r, r]^3, tau = coarse(T_p) + d, zero where
 *   x + tau leaves the box (so exactly 0 for any |tau_k| >= L); lig' = dlpd_rotate_trilinear(lig, R_p, center), or lig itself
 *   for R = null.  T (P, 3) int32 signed translations in voxels of the grid of scale * L points per edge;
 *   coarse(t) = floor(t / scale) (coarse_mode 0: what the global search's nearest upsample, DockingModels.py:74-76, is on the
 *   wrapped grid -- corr is then that search's correlation volume at (T_p + scale d) mod 2 scale L) or trunc(t / scale)
 *   (coarse_mode 1: the int() of MultiplyVolumes.py:56-58).
 * rec, lig (C, L^3) with per-pose strides in floats (0: one set for all poses); any 2 <= L <= 128, any C, 0 <= r <= 3.
 * ws: dlpd_local_ws_bytes(P, C, L, r) bytes (per-block partial sums, added in a fixed order: bit-reproducible). */
size_t dlpd_local_ws_bytes(int P, int C, int L, int r);
/* poses ONE dlpd_local_correlate call takes at most (a launch holds < 2^32 threads: one block per pose, channel and slab of
 * x-planes); more is DLPD_ERR_UNSUPPORTED -- the caller batches.  0 for an unsupported shape. */
int dlpd_local_max_poses(int C, int L);
int dlpd_local_correlate(const float* rec, const float* lig, const float* R, const int* T, float* corr, void* ws, int P, int C,
                         int L, int r, int scale, int coarse_mode, float center, long long rec_pstride, long long lig_pstride,
                         void* stream);
/* The adjoint of dlpd_local_correlate (training: src/Training/LocalTrainer.py:81-144 differentiates MultiplyVolumes):
 *   grec[p,c,X] = sum_d gcorr[p,c,d] lig'_p[c, X - tau_p - d],  glig[p,c,x] = sum_d gcorr[p,c,d] rec[c, x + tau_p + d],
 *   tau_p = coarse(T_p), d over the window, a term that leaves the box is 0.  rec, lig, R, T, the strides, scale, coarse_mode and
 * center as the forward took them; gcorr (P, C, W^3).  grec / glig are laid out as rec / lig: (P, C, L^3) with that volume's
 * per-pose stride, or, for stride 0 (one volume for all poses), (C, L^3) = the sum over the poses, added in pose order.  Either
 * may be null (not wanted); both null is DLPD_ERR_ARG.  Every element is written (the caller need not clear them); no atomics
 * and no workspace: the same bits run to run.  With R the sample of lig' is recomputed (no rotated volume is stored); glig
 * with R -- the scatter adjoint of the trilinear gather -- is DLPD_ERR_UNSUPPORTED.  Limits as the forward; a gradient per
 * pose takes at most dlpd_local_max_poses(C, L) poses per call. */
int dlpd_local_correlate_grad(const float* rec, const float* lig, const float* R, const int* T, const float* gcorr, float* grec,
                              float* glig, int P, int C, int L, int r, int scale, int coarse_mode, float center,
                              long long rec_pstride, long long lig_pstride, void* stream);
/* Both with the ligand sampled at a per-pose offset (sub-voxel translations; off (P,3) as dlpd_rotate_trilinear_shift takes it):
 *   corr[p,c,d] = sum_x rec[c, x + tau] lig_c( (center + off_p) + R_p^T (x - center) ).
 * The arguments, workspace, limits and error codes of the plain entries, `off` after R; off null: the plain entry's bits; off
 * without R: DLPD_ERR_ARG; glig with R stays DLPD_ERR_UNSUPPORTED (dlpd_rotate_trilinear_shift_grad carries that gradient). */
int dlpd_local_correlate_shift(const float* rec, const float* lig, const float* R, const float* off, const int* T, float* corr,
                               void* ws, int P, int C, int L, int r, int scale, int coarse_mode, float center,
                               long long rec_pstride, long long lig_pstride, void* stream);
int dlpd_local_correlate_shift_grad(const float* rec, const float* lig, const float* R, const float* off, const int* T,
                                    const float* gcorr, float* grec, float* glig, int P, int C, int L, int r, int scale,
                                    int coarse_mode, float center, long long rec_pstride, long long lig_pstride, void* stream);
/* The filter of those poses (DockingModels.py:118-119; with clip / clash the search's DockingModels.py:74-83, Docker.py:226,232):
 * feat[d] = [clamp(corr0[:, d]), clamp(corr1[:, coarse(T_p + d) - coarse(T_p)])], score (P, W^3) = MLP(feat) * (clash < thr).
 * corr0 (P, C0, W^3) from dlpd_local_correlate(scale 1, r); corr1 (P, C1, Wc^3) from dlpd_local_correlate(scale, rc)
 * on the coarse grid, rc = (r + 1) / 2 for scale 2 and r for scale 1, or null; clash (P, W^3) the forbidden volumes' correlation, or null; T on the FINE grid; scale 1 or 2.
 * W1t (C0 + C1, HP), b1 (HP), W2 (HP) padded to HP = dlpd_hidden_pad(H); a wider filter is DLPD_ERR_UNSUPPORTED (the caller
 * applies its module to the features).  best_score / best_index (P; either may be null): the minimum of each pose's window
 * and its flat index, lowest index on a tie (torch.min in Docker.update_top, Docker.py:89-98). */
int dlpd_local_filter(const float* corr0, int C0, const float* corr1, int C1, const float* clash, const int* T, int P, int r,
                      int scale, int coarse_mode, const float* W1t, const float* b1, const float* W2, float b2, int HP,
                      int has_clip, float clip, float thr, float* score, float* best_score, int* best_index, void* stream);

/* Stage K3, plain: real correlation volumes out (nb, CT, N^3) [+ clamp to +-clip]
 * (output of VolumeConvolution(clip), DockingModels.py:48,71). */
int dlpd_zifft_real(const void* wsB, float* out, int nb, int CT, int L, int has_clip, float clip,
                    void* stream);

/* Stage K3, fused scoring: z C2R + clip + SimpleFilter MLP (DockingModels.py:28-32,79-83) +
 * clash mask and multiply (Docker.py:226,232).  W1t (C,HP) transposed zero-padded first layer,
 * b1 (HP), W2 (HP).  V (nb, N^3). */
int dlpd_zifft_filter(const void* wsB, float* V, int nb, int C, int has_clash, int L, const float* W1t,
                      const float* b1, const float* W2, float b2, int HP, int has_clip, float clip,
                      float thr, void* stream);

/* Same for the reference's two-resolution layout (ProteinRepresentationModels.py:72-76): the Caux
 * channels of the coarser resolution arrive as clipped real correlation volumes aux (nb, Caux, L^3)
 * (grid N/2 = L) and are nearest-upsampled by index (DockingModels.py:74-76); W1t has C + Caux rows.
 * aux_is_preact: aux is (nb, HP, L^3) from dlpd_filter_preact -- the coarse half of the (linear) first
 * layer, bias included, evaluated once per coarse voxel -- and seeds the hidden units instead. */
int dlpd_zifft_filter_aux(const void* wsB, float* V, int nb, int C, int has_clash, int L, const float* W1t,
                          const float* b1, const float* W2, float b2, int HP, int has_clip, float clip,
                          float thr, const float* aux, int Caux, int aux_is_preact, void* stream);

/* One batch of the hot loop, Docker.py:211-232 (single-resolution model): K1 + K2 + K3. */
int dlpd_score_rotations(const float* lig, const void* recF, const float* R, int nb, int C, int has_clash,
                         int L, float center, const float* W1t, const float* b1, const float* W2, float b2,
                         int HP, int has_clip, float clip, float thr, void* wsA, void* wsB, float* V,
                         void* stream);

/* dlpd_score_rotations with oriented slabs (see dlpd_zfft_oriented). */
int dlpd_score_rotations_oriented(const float* lig, const void* recF, const float* R, int nb, int C, int has_clash,
                                  int L, float center, const float* W1t, const float* b1, const float* W2, float b2,
                                  int HP, int has_clip, float clip, float thr, void* wsA, void* wsB, float* V,
                                  int transposed, void* stream);

/* Per-voxel filter over materialised correlation volumes incl. nearest upsample of a second,
 * coarser resolution (DockingModels.py:74-83) and mask multiply (Docker.py:232). */
int dlpd_filter_mask(const float* conv0, int C0, int N0, const float* conv1, int C1, int N1,
                     const float* mask_norm, float thr, int has_clash, const float* W1t, const float* b1,
                     const float* W2, float b2, int H, float* V, int nb, void* stream);

/* The BACKWARD of that filter without the clash mask (the reference trains GlobalDockingModel's filter through torch's
 * interpolate / cat / permute / Linear / ReLU / Linear, DockingModels.py:74-83) for an incoming gradient g (nb, N0^3):
 *   pre_j = b1_j + sum_c W1[j,c] x_c is recomputed per fine voxel (x: the conv0 channels, then the conv1 channels at the
 *   coarse parent), delta_j = g W2_j [pre_j > 0];
 *   gconv0 (nb, C0, N0^3) = sum_j W1[j,c] delta_j;   gconv1 (nb, C1, N1^3) the same over the fine children of a coarse voxel;
 *   gparams = [gW1t (C x H) | gb1 (H) | gW2 (H) | gb2 (1)], sums over all nb N0^3 voxels, C = C0 + C1.
 * An output whose pointer is null is not computed (ws may be null without gparams).  Nothing is saved by the forward: the
 * inputs are all it reads.  Supported (the _supported call; DLPD_ERR_UNSUPPORTED otherwise): 1 <= H <= 64, C0 >= 1, C1 = 0
 * or N1 = N0 or N1 = N0 / 2 with N0 even, C0 + C1 <= 128, any N0 >= 2.  The voxels are split over a number of blocks that
 * depends on the shape alone, each writes its partial gparams to ws (the _ws_bytes call) and the partials are added in
 * ascending order in float64: no float atomics, the same bits on every run and device. */
int dlpd_filter_grad_supported(int C0, int N0, int C1, int N1, int H);
size_t dlpd_filter_grad_ws_bytes(int C0, int N0, int C1, int N1, int H, int nb);
int dlpd_filter_grad(const float* g, const float* conv0, int C0, int N0, const float* conv1, int C1, int N1,
                     const float* W1t, const float* b1, const float* W2, int H, float* gconv0, float* gconv1,
                     float* gparams, void* ws, int nb, void* stream);

/* Same with strided layouts and weights padded to HP = dlpd_hidden_pad(H): 4 voxels per thread,
 * float4 traffic.  conv0 (nb, *, N0^3) uses its first C0 channels (batch stride conv0_bstride);
 * mask_norm has batch stride mask_bstride (so it may be a channel of conv0).
 * conv1_is_preact: conv1 is (nb, HP, N1^3) from dlpd_filter_preact instead of (nb, C1, N1^3). */
int dlpd_filter_volumes(const float* conv0, int C0, long long conv0_bstride, int N0, const float* conv1, int C1,
                        int N1, int conv1_is_preact, const float* mask_norm, long long mask_bstride, float thr, int has_clash,
                        const float* W1t, const float* b1, const float* W2, float b2, int HP, float* V, int nb,
                        void* stream);

/* The coarse-resolution half of SimpleFilter's first layer (DockingModels.py:28, after the concat of
 * :77) evaluated on the coarse grid: pre (nb, HP, N1^3) = b1 + W1rows^T conv1, W1rows (C1, HP) = the
 * rows of W1t that belong to the coarse channels.  The first layer is linear, so upsampling these
 * HP planes by index equals applying it to the upsampled channels (8x fewer multiply-adds). */
int dlpd_filter_preact(const float* conv1, int C1, int N1, const float* W1rows, const float* b1, int HP,
                       float* pre, int nb, void* stream);

/* dlpd_zifft_filter_aux that also feeds the candidate lists of the top-K stage (dlpd_topk_select_cand): every score
 * whose order-preserving key is <= *tau is appended to the rotation's list cand_keys (nb, cap) u64 (key << 32 | flat
 * index), counted in cand_count[0..nb); *tau == 0 ("no valid filter yet", see dlpd_topk_merge_tau) flags the rotation
 * in cand_count[nb..2nb) for the full select instead.  tau / cand_keys / cand_count null: plain dlpd_zifft_filter_aux.
 * Replaces nothing in the reference: it is Docker.update_top's pick loop (Docker.py:89-98) seen from the producer. */
int dlpd_zifft_filter_cand(const void* wsB, float* V, int nb, int C, int has_clash, int L, const float* W1t,
                           const float* b1, const float* W2, float b2, int HP, int has_clip, float clip, float thr,
                           const float* aux, int Caux, int aux_is_preact, const void* tau, void* cand_keys,
                           void* cand_count, int cap, void* stream);

/* dlpd_zifft_filter_cand with the kernel formulation named (same arithmetic, bit-identical V): form 0 = the
 * library's default, 1 = every wave owns a channel of the group and the transform / filter phases alternate behind
 * block barriers, 2 = role-split blocks -- dedicated transform waves (LDS-DMA, pack, z C2R) and filter waves (the
 * MLP of DockingModels.py:79-83 from registers) that overlap each other; falls back to 1 where 2 is not compiled.
 * libdlpd.so holds ONE formulation per box -- 1 at boxes 32 / 40, 2 at boxes 64 / 80; form 1 at boxes 64 / 80 (and raw
 * aux channels there, aux_is_preact = 0) is DLPD_ERR_UNSUPPORTED unless the library was built with -DDLPD_TEST_VARIANTS
 * (tests/variants: the bit-exactness reference of the tests). */
int dlpd_zifft_filter_form(const void* wsB, float* V, int nb, int C, int has_clash, int L, const float* W1t,
                           const float* b1, const float* W2, float b2, int HP, int has_clip, float clip, float thr,
                           const float* aux, int Caux, int aux_is_preact, const void* tau, void* cand_keys,
                           void* cand_count, int cap, int form, void* stream);

/* Stage K3 for the COARSER resolution of a two-resolution model: z C2R + clip fused with that resolution's half of
 * SimpleFilter's first layer (DockingModels.py:28 after the concat of :77, linear): pre (nb, HP, N^3) = b1 +
 * W1rows^T clamp(corr), W1rows (C, HP) = the rows of W1t that belong to these channels.  The fine grid's
 * dlpd_zifft_filter_aux(aux = pre, aux_is_preact = 1) picks the planes up by index (nearest upsample, :74-76);
 * the C real correlation volumes of this resolution are never written. */
int dlpd_zifft_preact(const void* wsB, float* pre, int nb, int C, int L, const float* W1rows, const float* b1, int HP,
                      int has_clip, float clip, void* stream);
/* dlpd_zifft_preact with the kernel formulation named (see dlpd_zifft_filter_form). */
int dlpd_zifft_preact_form(const void* wsB, float* pre, int nb, int C, int L, const float* W1rows, const float* b1,
                           int HP, int has_clip, float clip, int form, void* stream);

/* dlpd_zifft_real with the clamp restricted to channels [0, nclip). */
int dlpd_zifft_real_part(const void* wsB, float* out, int nb, int CT, int nclip, int L, int has_clip, float clip,
                         void* stream);

/* Representation-plugin convolution (ProteinRepresentationModels.py:85-114, the per-batch cost of
 * Docker.dockE3, Docker.py:166-167): y (B, cout, D^3) = [relu] conv3d(x (B, cin, D^3), w (cout, cin, ks^3)),
 * padding ks/2, stride 1, no bias, exact f32 on the matrix cores.  Supported: ks in {3,5}, cout a multiple
 * of 16, D <= 80 (dlpd_conv3d_supported); anything else is the plugin's own torch convolution. */
int dlpd_conv3d_supported(int cin, int cout, int ks, int D);
/* weights are passed packed: wp = dlpd_conv3d_pack(w (cout, cin, ks^3)), dlpd_conv3d_packed_floats() floats */
size_t dlpd_conv3d_packed_floats(int cin, int cout, int ks);
int dlpd_conv3d_pack(const float* w, float* wp, int cin, int cout, int ks, void* stream);
int dlpd_conv3d(const float* x, const float* wp, float* y, int B, int cin, int cout, int D, int ks, int relu,
                void* stream);
/* Same with stride 1 or 2 (padding ks/2): the stride-2 layer of SE3MultiResReprScalar
 * (ProteinRepresentationModels.py:51).  y (B, cout, Do^3), Do = (D - 1) / stride + 1. */
int dlpd_conv3d_strided(const float* x, const float* wp, float* y, int B, int cin, int cout, int D, int ks, int relu,
                        int stride, void* stream);

/* The same convolution on the BF16 matrix cores with f32-grade results: inputs and weights are split into three bf16
 * terms each and every product is summed from six bf16 products in f32 (the three dropped ones are below f32's own
 * rounding): 16 / 6 = 2.7 x the matrix throughput of the exact-f32 form, results equal to it to a few 1e-7 relative.
 * Weights are passed packed AND split: wp = dlpd_conv3d_split_pack(w (cout, cin, ks^3)), dlpd_conv3d_split_packed_bytes()
 * bytes.  Same supported shapes as dlpd_conv3d (dlpd_conv3d_supported); stride 1 or 2.  Replaces the same reference
 * lines (ProteinRepresentationModels.py:85-114, Docker.py:166-167). */
size_t dlpd_conv3d_split_packed_bytes(int cin, int cout, int ks);
int dlpd_conv3d_split_pack(const float* w, void* wp, int cin, int cout, int ks, void* stream);
int dlpd_conv3d_split(const float* x, const void* wp, float* y, int B, int cin, int cout, int D, int ks, int relu,
                      int stride, void* stream);
/* Tile occupancy: the plugins' convolutions have no bias (ProteinRepresentationModels.py:85-96: bias=False), so an output
 * tile whose receptive field is all zero is zero, and a protein fills a fraction of its box.  occ (B, ceil(D/4), ceil(D/4),
 * ceil(D/4)) bytes, non-zero where the 4 x 4 x 4 cell of the volume holds a non-zero value in some channel:
 * dlpd_conv3d_tile_occupancy computes it for any (B, cin, D^3) tensor; dlpd_conv3d_split_sparse skips the 4 x 4 x 16 output
 * tiles whose neighbouring input cells (a superset of the halo) are empty (occ_in; null = dense) and writes the map of ITS output (occ_out; null = none; not
 * written for stride 2) -- the next layer's occ_in.  Results are bit-identical to dlpd_conv3d_split.
 * unwritten != 0 (needs both maps, stride 1): the activations travel WITH their maps -- an output tile whose neighbourhood is
 * empty is not written at all (its cells stay 0 in occ_out) and no voxel of a cell that occ_in marks empty is read (it is
 * taken as the zero the map stands for): y holds the same values as before in every cell occ_out marks and is undefined
 * elsewhere; every consumer must go by the map (the next layer with unwritten != 0, dlpd_maxpool3d_5s2_sparse,
 * dlpd_zfft_volumes_occ).  Docker.dockE3's per-batch representation (Docker.py:163-167) spent most of its time writing the
 * zeros of skipped tiles. */
size_t dlpd_conv3d_tile_occupancy_bytes(int B, int D);
int dlpd_conv3d_tile_occupancy(const float* x, unsigned char* occ, int B, int cin, int D, void* stream);
int dlpd_conv3d_split_sparse(const float* x, const void* wp, float* y, const unsigned char* occ_in, unsigned char* occ_out,
                             int B, int cin, int cout, int D, int ks, int relu, int stride, int unwritten, void* stream);

/* The convolution's gradient with respect to its weights -- what L.backward() in the reference's trainer
 * (src/Training/LocalTrainer.py, optimize) asks of every Conv3d of the representation plugins:
 *   gw (cout, cin, ks^3) = sum over b and voxels v of gy (B, cout, D^3)[b, co, v] * x (B, cin, D^3)[b, ci, v + tap - ks/2]
 * for the stride-1 layer y = conv3d(x, w, padding ks/2), zeros outside the box; exact f32 products on the matrix cores, f32
 * accumulation.  Shapes: those of dlpd_conv3d_supported, any B; stride 2 is not supported.  The voxels are split over
 * `nparts` blocks in a fixed order (block p takes the patches p, p + nparts, ...), each writes its partial gw to ws
 * (dlpd_conv3d_wgrad_ws_floats() floats) and the partials are added in ascending p: no float atomics, the same bits for the
 * same nparts on every run and device.  (The gradient with respect to x is dlpd_conv3d / dlpd_conv3d_split on gy with the
 * flipped, transposed weights.) */
size_t dlpd_conv3d_wgrad_ws_floats(int cin, int cout, int ks, int nparts);
int dlpd_conv3d_wgrad(const float* x, const float* gy, float* gw, float* ws, int B, int cin, int cout, int D, int ks,
                      int nparts, void* stream);

/* MaxPool3d(kernel 5, stride 2, padding 2) of the E3 plugin (ProteinRepresentationModels.py:101):
 * x (nvol, D^3) -> y (nvol, Do^3), Do = (D - 1) / 2 + 1. */
int dlpd_maxpool3d_5s2(const float* x, float* y, int nvol, int D, void* stream);
/* The same with occupancy maps (dlpd_conv3d_tile_occupancy): x (B, C, D^3); occ_in (the input's cells; null = read everything):
 * output tiles whose inputs lie in empty cells are written as +0.0 without reading them; occ_out (null = none): the cells of
 * the (B, C, Do^3) output that hold a non-zero value in some channel -- the next convolution's occ_in.
 * unwritten != 0 (needs occ_in): as dlpd_conv3d_split_sparse -- input voxels of empty cells are not read (zero), output tiles
 * over empty cells are not written. */
int dlpd_maxpool3d_5s2_sparse(const float* x, float* y, const unsigned char* occ_in, unsigned char* occ_out, int B, int C, int D,
                              int unwritten, void* stream);

/* Docker.update_top pick loop, src/Docker/Docker.py:89-98: per rotation the K picks in pick order
 * (incl. the zero-fill behaviour).  V (nb, nvox); out (nb, K). */
size_t dlpd_topk_workspace_bytes(int nb, int K);
int dlpd_topk_select(const float* V, int nb, long long nvox, int K, float* out_score, int* out_idx,
                     void* ws, void* stream);

/* dlpd_topk_select with the candidate lists K3 filled for this batch (dlpd_zifft_filter_cand).  Once the running list
 * is full and its K-th score negative, a later pick can enter it only with a score <= that K-th score, and every
 * voxel of a rotation scoring below a candidate is a candidate too, so a candidate's rank in its sorted list IS its
 * pick order: rotations with a complete list (flag clear, count <= cap) skip the radix select over V; the others take
 * it as before.  Consumes the lists and resets cand_count.  cap in [64, 8192]. */
int dlpd_topk_select_cand(const float* V, int nb, long long nvox, int K, float* out_score, int* out_idx, void* ws,
                          const void* cand_keys, void* cand_count, int cap, void* stream);

/* Docker.update_top list maintenance, src/Docker/Docker.py:100-105: append, stable sort by score,
 * truncate -- on a device-resident list.  glist: u64 count, u64 pad, u64 hi[K], u64 lo[K] with
 * hi = score_key<<32 | rotation, lo = pick<<32 | negzero<<31 | flat_index. */
size_t dlpd_topk_glist_bytes(int K);
int dlpd_topk_glist_reset(void* glist, int K, void* stream);
int dlpd_topk_merge(const float* cand_score, const int* cand_idx, const int* rot_ids, int nb, int K,
                    void* glist, void* stream);
/* Same, publishing the candidate filter for the K3 launches of later batches: *tau_out (u32) = order-preserving key of
 * the list's K-th score once the list holds K entries and that score is negative, else 0. */
int dlpd_topk_merge_tau(const float* cand_score, const int* cand_idx, const int* rot_ids, int nb, int K,
                        void* glist, void* tau_out, void* stream);

/* Exclusion radius of the search.  BUILD-DEFINED, both entries: the reference clears ONE voxel per pick
 * (Docker.py:98) and has no counterpart; r = 0 -- neither call -- is the reference.  On the cubic grid of side n with flat
 * index (x n + y) n + z and an integer radius r >= 1: u BEATS v iff V[u] < V[v], or V[u] == V[v] and flat(u) < flat(v);
 * B_r(v) is the cyclic Chebyshev ball {(v + d) mod n : d in [-r, r]^3}.  suppress_r(V)[v] is V[v] itself where V[v] < 0 is
 * false (zeros, -0.0 and positives keep their bits), V[v] where V[v] < 0 and no other voxel of B_r(v) beats v, and +0.0 --
 * what a pick of the reference leaves in the voxel it took -- everywhere else.  The list of a search with exclusion r is
 * Docker.update_top run on suppress_r(V) for every rotation: pick order, the zero-fill behaviour and the merge key keep their
 * definitions, and no two negative entries of one rotation lie within r voxels of each other on the wrapped grid.  NaN scores
 * are outside the contract, as for the select.
 * dlpd_topk_suppress: Vs (nb, n^3) = suppress_r(V), never in place.  cand_count (null: every rotation; else the 2 nb words of
 *   dlpd_topk_select_cand): the rows of rotations whose candidate list is complete (flag clear, count <= cap) are NOT written
 *   -- the select reads Vs only for the rotations it radix-selects.
 * dlpd_topk_suppress_cand: every complete list loses the candidates that some voxel of their ball beats in V (whatever beats
 *   a candidate scores below it, so V is all the test needs); survivors keep their order, cand_count[b] is lowered;
 *   incomplete lists and the flags are left alone.  cap in [64, 8192].
 * Order within a launch: dlpd_topk_suppress (flags given), dlpd_topk_suppress_cand, dlpd_topk_select_cand on Vs.
 * r < 1, r > 4, 2 r + 1 > n, nb <= 0, a null pointer, V == Vs: DLPD_ERR_ARG; n^3 >= 2^31: DLPD_ERR_UNSUPPORTED; on an error
 * nothing is launched. */
int dlpd_topk_suppress(const float* V, float* Vs, int nb, int n, int r, const void* cand_count, int cap, void* stream);
int dlpd_topk_suppress_cand(const float* V, int nb, int n, int r, void* cand_keys, void* cand_count, int cap, void* stream);

/* Search under distance restraints.  BUILD-DEFINED, both entries: the reference has no counterpart; without
 * restraints -- neither call -- is the reference.  Poses as Docker.cluster / Docker.evaluate take them: list entry
 * (rot, x, y, z) carries a ligand point a (Angstrom, ligand centred on the origin) to R_rot a + resolution t, t the signed
 * translation of (x, y, z); a receptor point b is in Angstrom in the search frame (origin-centred, after randR).  Restraint
 * j = (a_j, b_j, dmin_j, dmax_j), 0 <= dmin <= dmax < inf, is satisfied iff dmin <= |R a + res t - b| <= dmax; a set is J
 * restraints (1..32) and a number need (1..J), and a pose is ALLOWED iff it satisfies at least `need` of them.
 * The predicate is evaluated in integers, in units of 1/256 voxel (0.005 A at 1.25 A: the step of the test).  The host
 * computes in float64 the centres c[rot][j] = round_half_even(256 (b_j - R_rot a_j) / resolution), int32 (nrot, J, 3),
 * |c| <= 2^20, and lo_j = round(256 dmin / res), hi_j = round(256 dmax / res) <= 2^21, stored squared as int64: bounds =
 * lo^2 of the J restraints, then hi^2.  For voxel v of the cubic grid of EVEN side n the signed index per axis is
 * t = v - n if v >= n / 2 else v (Docker.signed_translation with box_size = n / 2: on an embedded box the test is on the
 * reported pose), d^2 = sum over the axes of (256 t - c)^2 in int64, and the restraint is satisfied iff lo^2 <= d^2 <= hi^2,
 * both ends inclusive.  A centre outside the grid is legal; the restraint is then unsatisfiable for that rotation.
 * restrain(V)[v] is V[v] itself where V[v] < 0 is false (zeros, -0.0 and positives keep their bits) and where V[v] < 0 and v
 * is allowed, +0.0 everywhere else.  The list of a restrained search is Docker.update_top run on restrain(V) for every
 * rotation: every negative entry of the list is an allowed pose (zero-fill entries are outside that promise, as for the
 * exclusion radius).  With an exclusion radius as well the result is the intersection: a voxel survives iff it is a local
 * minimum of the UNRESTRICTED V and is allowed -- the two masks commute, and a rejected minimum still suppresses its
 * neighbours.
 * dlpd_topk_restrain: Vs (nb, n^3) = restrain(V); Vs == V is allowed.  rot_ids: the batch's global rotation indices, device
 *   int32 (the tensor dlpd_topk_merge gets); they index centres.  cand_count as for dlpd_topk_suppress: the rows of rotations
 *   whose candidate list is complete are NOT written.
 * dlpd_topk_restrain_cand: every complete list (flag clear, count <= cap) loses the candidates that are not allowed; survivors
 *   keep their order, cand_count[b] is lowered.  With tau (the word dlpd_topk_merge_tau publishes; null or *tau == 0: no
 *   rebuild) every OVERFLOWED list (flag clear, count > cap) is rebuilt from the bounding cubes of the J balls, clipped to the
 *   grid: every allowed voxel whose key is <= *tau, each once; if they are at most cap the list is complete and its count
 *   set, else the count stays above cap.  Flagged lists and the flags are left alone.  The caller bounds the summed volume
 *   of the cubes (one block walks them).  cap in [64, 8192].
 * Order within a launch: dlpd_topk_restrain_cand; dlpd_topk_suppress and dlpd_topk_suppress_cand when there is a radius (they
 * thin the rebuilt lists too); dlpd_topk_restrain (flags given; in place on Vs after a suppress, V -> Vs otherwise);
 * dlpd_topk_select_cand on Vs.  Without candidate lists: dlpd_topk_restrain, then dlpd_topk_select on Vs.
 * An odd n, J outside [1, 32], need outside [1, J], nb <= 0, a null required pointer, cap outside [64, 8192] (cand entry):
 * DLPD_ERR_ARG; n^3 >= 2^31: DLPD_ERR_UNSUPPORTED; on an error nothing is launched. */
int dlpd_topk_restrain(const float* V, float* Vs, int nb, int n, const int* rot_ids, const int* centres,
                       const long long* bounds, int J, int need, const void* cand_count, int cap, void* stream);
int dlpd_topk_restrain_cand(const float* V, int nb, int n, const int* rot_ids, const int* centres,
                            const long long* bounds, int J, int need, const void* tau, void* cand_keys, void* cand_count,
                            int cap, void* stream);

/* Pose clustering of a finished list.  BUILD-DEFINED, all four entries: the reference has no counterpart and no call site
 * (Docker.cluster is this build's own step after the search).  A rigid pose p = (R_p, t_p) of one ligand is handed over as
 * its embedding e_p, 12 floats (ops.pose_embedding): the RMSD between two poses over the ligand's (weighted) atoms is the
 * Euclidean distance of their embeddings.  Every squared distance is one fma chain over the twelve differences in a fixed
 * order, so d(i, j) and d(j, i) have the same bits and equal poses give exactly 0.  K, Ka, Kb <= 65536 (else
 * DLPD_ERR_UNSUPPORTED); K <= 0, a null pointer, a negative or NaN radius, a short workspace: DLPD_ERR_ARG; on an error
 * nothing is launched and nothing is written.
 * dlpd_pose_rmsd: D (Ka, Kb) = d(Ea[i], Eb[j]).
 * dlpd_pose_within: the neighbour bitmap alone -- mask holds K rows of W = ceil(K / 64) 64-bit words, row-major: bit (j & 63)
 *   of mask[i * W + (j >> 6)] is set iff d(i, j)^2 <= radius^2 in float32; bits of columns >= K are zero.
 * dlpd_pose_cluster: the greedy clustering of the list in its own order (best first).  Pose i is a centre iff no earlier
 *   centre lies within radius of it; every other pose belongs to the first centre within radius.  The scan stops after
 *   max_clusters centres (<= 0 or > K: no limit); a pose none of them covers gets label -1.  centres / sizes: the first *count
 *   entries are written (room for min(K, max_clusters)); labels (K); count (1); all int32 on the device.  ws: the bitmap,
 *   dlpd_pose_cluster_ws(K) = K * ceil(K / 64) * 8 bytes (0 for an unsupported K), 8-byte aligned; it never leaves the
 *   device.  Integer work once the bitmap stands: the same input gives the same bytes. */
int dlpd_pose_rmsd(const float* Ea, const float* Eb, float* D, int Ka, int Kb, void* stream);
int dlpd_pose_within(const float* E, int K, float radius, void* mask, void* stream);
size_t dlpd_pose_cluster_ws(int K);
int dlpd_pose_cluster(const float* E, int K, float radius, int max_clusters, int* centres, int* sizes, int* labels, int* count,
                      void* ws, size_t ws_bytes, void* stream);

/* Evaluation of a list of poses against a native complex: what the reference's EvaluateBenchmark.py:95-113
 * (interface RMSD) and processing_utils.py:183-236 (contacts, fnat, CAPRI class) compute pose by pose on the host.  A pose
 * is 12 doubles, R row-major then t in Angstrom: it carries the bbox-centred unbound ligand's point y to R y + t, next to the
 * bbox-centred unbound receptor (the frame of a .dat file).  K <= 65536, nI <= 16, NLa <= 2048, NRa <= 65536, C <= 65536
 * (else DLPD_ERR_UNSUPPORTED); a null pointer, K <= 0, nI <= 0, a record with nl < 1 or nr < 0, a contact whose atom range is
 * empty or leaves its array, a negative or NaN cutoff: DLPD_ERR_ARG; on an error nothing is launched and nothing is written.
 * dlpd_pose_native_rmsd: moments holds nI interface records and then the L-RMSD record, 48 doubles each, on the device
 *   (layout and formulas: csrc/dlpd_evaluate.h; packed by ops.native_moments); counts is a HOST array of (nI + 1) x (nr, nl)
 *   int32, the point counts of the records (nr of the last is ignored).  irmsd[k] = the minimum over the nI pairs of the
 *   superposed RMSD, lrmsd[k] = the RMSD of the ligand's points to their targets without superposition; all float64.
 * dlpd_pose_native_contacts: rec_atoms (NRa, 3) / lig_atoms (NLa, 3) float32, residue-contiguous; contact c is the atom
 *   ranges rec [r0, r1) x lig [l0, l1), ranges = (C, 4) int32 (r0, r1, l0, l1) on the device and ranges_host the same values in
 *   host memory (the copy that is checked).  count[k] (int32) = the contacts with an atom pair at d^2 <= cutoff^2 in float32
 *   under pose k (R, t rounded to float32 once).  C = 0 is allowed (every count 0).
 * dlpd_pose_capri: fnat[k] = count[k] / (C + 0.001) (float64) and capri[k] (int32), the class cascade on (fnat, lrmsd, irmsd). */
int dlpd_pose_native_rmsd(const double* poses, int K, const double* moments, const int* counts, int nI, double* irmsd, double* lrmsd,
                          void* stream);
int dlpd_pose_native_contacts(const double* poses, int K, const float* rec_atoms, int NRa, const float* lig_atoms, int NLa,
                              const int* ranges, const int* ranges_host, int C, float cutoff, int* count, void* stream);
int dlpd_pose_capri(const int* count, const double* irmsd, const double* lrmsd, int C, int K, double* fnat, int* capri, void* stream);

/* Every residue contact of the posed complex: the ``dec`` set that processing_utils.py:183-216 finds per decoy
 * with a neighbour search over all atoms of both proteins, counted, and its overlap with the native set -- the two integers
 * fnonnat = (n_dec - n_corr) / (n_dec + 0.001) (_get_fnat, :219-224) is made of.  Poses and frames as above.
 * rec_atoms (NRa, 3) / lig_atoms (NLa, 3) float32: ALL atoms, residue-contiguous; rec_off (NRres + 1) / lig_off (NLres + 1)
 * int32: residue i owns atoms [off[i], off[i + 1]); rec_off_host / lig_off_host: the same values in host memory (the copies that
 * are checked: non-decreasing, inside the arrays).  rec_sph (NRres, 4) / lig_sph (NLres + 1, 4) float32: per residue a centre
 * and a radius, rounded up, that covers its atoms; the last row of lig_sph covers the whole ligand; lig_extent >= |y|_2 of
 * every ligand atom and centre (what the filter's padding is derived from: csrc/dlpd_contacts.h).  native_bits: the native
 * pairs as a bitmap, bit (rho & 31) of word lambda * ceil(NRres / 32) + (rho >> 5), NLres * ceil(NRres / 32) words.
 * n_dec[k] = the residue pairs (rho, lambda) with an atom pair at d^2 <= cutoff^2 in float32 under pose k -- the predicate of
 * dlpd_pose_native_contacts, bit for bit -- and n_corr[k] = those of them whose bit is set (both int32).
 * K <= 65536, NLa <= 8192, NLres <= 1024, NRa <= 65536, NRres <= 8192 (else DLPD_ERR_UNSUPPORTED); a null pointer, K < 0, an
 * empty structure, offsets out of order, a negative or NaN cutoff or extent: DLPD_ERR_ARG; K = 0 is a no-op.  On an error
 * nothing is launched and nothing is written. */
int dlpd_pose_contacts_all(const double* poses, int K, const float* rec_atoms, const int* rec_off, const float* rec_sph, int NRa,
                           int NRres, const float* lig_atoms, const int* lig_off, const float* lig_sph, int NLa, int NLres,
                           const int* rec_off_host, const int* lig_off_host, const unsigned* native_bits, float lig_extent,
                           float cutoff, int* n_dec, int* n_corr, void* stream);

/* The interface of every pose as residue bitmaps, and two consumers of them.  BUILD-DEFINED, all five entries: the
 * reference has no counterpart.  On an error nothing is launched and nothing is written; K = 0 is a no-op everywhere.
 * dlpd_pose_residue_bits: the arguments, frames, predicate, limits and checks of dlpd_pose_contacts_all without the native bitmap.
 *   rec_bits (K, Wr) / lig_bits (K, Wl) uint32 on the device, Wr = ceil(NRres / 32), Wl = ceil(NLres / 32): bit (i & 31) of word
 *   i >> 5 of row k is set iff residue i has an atom at d^2 <= cutoff^2 in float32 of some atom of the partner under pose k.  Every
 *   word of every row is written; the bits at and above NRres / NLres are zero.
 * dlpd_interface_profile: over the K rows of the two bitmaps, rec_count / lig_count (int32) = the poses that mark a residue and
 *   rec_freq / lig_freq (float64) = the sum of weights[k] (K float64 on the device, any values) over those poses.  The order of the
 *   sum depends on K alone: poses in chunks of 1,024, ascending within a chunk from +0, a set bit adds weights[k] (no product);
 *   the chunk partials are added in ascending order starting from the first.  ws: the partials,
 *   dlpd_interface_profile_ws(K, NRres, NLres) bytes (0 for unsupported sizes), 8-byte aligned.  K <= 65536, NRres <= 8192,
 *   NLres <= 1024 (else DLPD_ERR_UNSUPPORTED); a null pointer, K < 0, no residues, a short workspace: DLPD_ERR_ARG.
 * dlpd_interface_within: a pose's fingerprint F is its Wr + Wl words (either may be 0, not both; the bitmap of a side with no
 *   words may be null).  mask has the layout of dlpd_pose_within: bit (j & 63) of mask[i * W + (j >> 6)], W = ceil(K / 64), is set
 *   iff |F_i & F_j| * 1024 >= q * |F_i | F_j| -- integers only; two empty fingerprints are neighbours, the diagonal is set, the
 *   bitmap is symmetric; bits of columns >= K are zero.  K <= 65536, Wr <= 256, Wl <= 32 (else DLPD_ERR_UNSUPPORTED); a null
 *   pointer, a negative size, q outside 0..1024: DLPD_ERR_ARG.
 * dlpd_interface_cluster: that bitmap, then the greedy scan of dlpd_pose_cluster on it, with that entry's outputs, max_clusters
 *   and workspace: dlpd_pose_cluster_ws(K) bytes; the bitmap never leaves the device. */
int dlpd_pose_residue_bits(const double* poses, int K, const float* rec_atoms, const int* rec_off, const float* rec_sph, int NRa,
                           int NRres, const float* lig_atoms, const int* lig_off, const float* lig_sph, int NLa, int NLres,
                           const int* rec_off_host, const int* lig_off_host, float lig_extent, float cutoff, unsigned* rec_bits,
                           unsigned* lig_bits, void* stream);
size_t dlpd_interface_profile_ws(int K, int NRres, int NLres);
int dlpd_interface_profile(const unsigned* rec_bits, const unsigned* lig_bits, int K, int NRres, int NLres, const double* weights,
                           double* rec_freq, double* lig_freq, int* rec_count, int* lig_count, void* ws, size_t ws_bytes, void* stream);
int dlpd_interface_within(const unsigned* rec_bits, const unsigned* lig_bits, int K, int Wr, int Wl, int q, void* mask, void* stream);
int dlpd_interface_cluster(const unsigned* rec_bits, const unsigned* lig_bits, int K, int Wr, int Wl, int q, int max_clusters,
                           int* centres, int* sizes, int* labels, int* count, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
