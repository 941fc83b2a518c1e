// ccp_grid_mg_view.hpp — what the multigrid solver (ccp_grid_mg.hip) needs of a grid handle (ccp_grid.hip owns the
// handle, ccp_grid_mg.hip the hierarchy cached on it).  Declarations only: no kernels.
#pragma once

#include "ccp_grid_stencil.hpp"

namespace ccp {

struct MgHierarchy;
void mg_release(MgHierarchy *h);

// CCP_MG_NULLSPACE_* (ccp_grid_mg_set_nullspace) and what the handle remembers for it: the census verdict of the
// installed operators (-1: not taken yet, 0: one is not floating, 1: all are) and ccp_grid_mg_nullspace_info's figures of
// every channel's last CONSTANT-mode solve.  A new operator forgets the verdict and the figures.
struct MgNullspace {
    int kind = 0;
    int floating = -1;
    bool solved[kMaxChannels] = {};
    double b_mean[kMaxChannels] = {}, x_mean[kMaxChannels] = {};
    void forget()
    {
        floating = -1;
        for (bool &s : solved) s = false;
    }
};

struct GridMgView {
    Geom geom;
    int channels;
    bool masked;
    bool one_block;                  // no ghost rows: the whole image in this handle
    double *x, *b;
    const unsigned char *mask;
    // a weighted handle (CCP_GRID_WEIGHTED): its level-0 planes d, we, ws, lambda in the layout of one channel of x, all
    // null while it has no operator
    bool weighted;
    const double *wd, *wwe, *wws, *wlam;
    // one operator per channel (ccp_grid_set_weights_per_channel_device): op_channels == channels sets of those planes,
    // channel ch's d, we, ws at + ch * op_stride and its lambda at + ch * lam_stride; the shared operator: op_channels 1
    int op_channels;
    long op_stride, lam_stride;
    int hierarchy_kind;              // CCP_MG_HIERARCHY_* (ccp_grid_mg_set_hierarchy; GALERKIN unless the handle is weighted)
    int precision;                   // CCP_MG_PRECISION_* (ccp_grid_mg_set_precision)
    int channels_mode;               // CCP_MG_CHANNELS_* (ccp_grid_mg_set_channels)
    int smoother;                    // CCP_MG_SMOOTHER_* (ccp_grid_mg_set_smoother)
    MgNullspace *ns;                 // ccp_grid_mg_set_nullspace's value, the census verdict and the last solves' means
    hipStream_t stream;
    int device;                      // the handle's device (what a ccp_device_array argument is checked against)
    MgHierarchy **cache;            // the handle's cached hierarchy (built on first use, dropped with the mask and the partition)
    // row blocks (ccp_grid_attach_comm): the communicator, every rank's first image row then the image height
    // (world + 1 entries), and the handle's ghost depth; comm is null when none is attached
    ccp_comm *comm;
    const int *part;
    int ghost;
};
int grid_mg_view(ccp_grid *g, GridMgView *v);
// the handle's hierarchy kind (ccp_grid_mg_set_hierarchy / _get_hierarchy) and whether the handle is weighted
int grid_mg_hierarchy_slot(ccp_grid *g, bool *weighted, int **kind, MgHierarchy ***cache);
// the handle's V-cycle precision (ccp_grid_mg_set_precision / _get_precision) and whether the handle is a row block
int grid_mg_precision_slot(ccp_grid *g, int **precision, MgHierarchy ***cache, bool *row_block);
// the handle's channel mode (ccp_grid_mg_set_channels / _get_channels)
int grid_mg_channels_slot(ccp_grid *g, int **mode, MgHierarchy ***cache);
// the handle's smoother (ccp_grid_mg_set_smoother / _get_smoother)
int grid_mg_smoother_slot(ccp_grid *g, int **kind, MgHierarchy ***cache);
// the handle's null-space record (ccp_grid_mg_set_nullspace / _get_nullspace) and whether the handle is weighted
int grid_mg_nullspace_slot(ccp_grid *g, bool *weighted, MgNullspace **ns);
void grid_mg_halo_stale(ccp_grid *g);   // after a row-block solve: the next sweep refreshes the ghost rows first

}  // namespace ccp
