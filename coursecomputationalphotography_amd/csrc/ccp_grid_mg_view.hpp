// ccp_grid_mg_view.hpp — what the multigrid solver (ccp_grid_mg.hip) needs of a grid handle (ccp_grid_handle.hpp defines the
// handle, ccp_grid_mg.hip the hierarchy cached on it).  Declarations only: no kernels.
#pragma once

#include "ccp_grid_stencil.hpp"

namespace ccp {

struct MgHierarchy;
void mg_release(MgHierarchy **cache);   // deletes the cached hierarchy, if any, and leaves null

// The multigrid options of a handle, CCP_MG_*_* each (ccp_grid_mg_set_* / _get_*).  They outlive every operator, mask and
// communicator the handle is given; what a change of one frees of the cached hierarchy: kOptions (ccp_grid_mg.hip).
struct MgConfig {
    int hierarchy = CCP_MG_HIERARCHY_GALERKIN;   // (weighted handles only: the others keep the default)
    int precision = CCP_MG_PRECISION_F64;
    int channels = CCP_MG_CHANNELS_SEQUENTIAL;
    int smoother = CCP_MG_SMOOTHER_POINT;
    int nullspace = CCP_MG_NULLSPACE_NONE;       // (weighted handles only)
    bool operator==(const MgConfig &o) const
    {
        return hierarchy == o.hierarchy && precision == o.precision && channels == o.channels && smoother == o.smoother && nullspace == o.nullspace;
    }
};

// What the handle remembers for CCP_MG_NULLSPACE_CONSTANT: the census verdict of the installed operators (-1: not taken
// yet, 0: one is not floating, 1: all are) and ccp_grid_mg_nullspace_info's figures of every channel's last solve in that
// mode.  A new operator forgets the verdict and the figures.
struct MgNullspace {
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
    MgConfig cfg;                    // the handle's options, by value
    MgNullspace *ns;                 // the census verdict and the last CONSTANT-mode solves' means
    // ccp_grid_refresh_weights_device: was the last change of the operator a refresh; *op_status (device; null unless the
    // handle is weighted) is its CCP_OPERATOR_* word, 0 while the last change was a setter's, which the fold kernel forms
    // from op_verdict[0] (device: the refresh pass's weight verdict), the narrowing's flag and the census counts
    bool refreshed;
    unsigned *op_status;
    unsigned long long *op_verdict;
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
// What the option setters and getters work on: the options themselves, the cached hierarchy, and the two facts a setter
// may refuse on (row_block: the handle has ghost rows or holds fewer rows than the image)
struct GridMgSlot {
    MgConfig *cfg;
    MgHierarchy **cache;
    bool weighted, row_block;
};
int grid_mg_slot(ccp_grid *g, GridMgSlot *s);
void grid_mg_halo_stale(ccp_grid *g);   // after a row-block solve: the next sweep refreshes the ghost rows first

}  // namespace ccp
