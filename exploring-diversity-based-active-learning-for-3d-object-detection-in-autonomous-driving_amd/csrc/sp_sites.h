// Internal (not part of the C ABI): the site-numbering passes of al3d_sp_down_sites (csrc/spconv.hip) for other marking rules.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// `workspace` (>= al3d_sp_down_sites_workspace_bytes(B, OD, OH, OW), 16-byte aligned) starts with one flag byte (0 | 1) per
// cell of the [B][OD][OH][OW] grid, padded with zeros to a multiple of 32 bytes.  Numbers the flagged cells in raster
// (b, z, y, x) order: grid_out[cell] = row, coords_out[row] = (b, z, y, x) for row < cap, *counter = the count.
int al3d_sp_number_marked_raster(void* workspace, int B, int OD, int OH, int OW, int* grid_out, int* coords_out, int* counter,
                                 int cap, hipStream_t stream);
