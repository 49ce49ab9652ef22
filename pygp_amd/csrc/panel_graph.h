// Host side of the task-queue launches (panel_graph.hip): the task graph of a panel, its
// order, the lists the launches copy to the device and the rules that size their grids.
// No kernel and no call into the HIP runtime.
#pragma once

#include "panel_task.h"

#include <vector>

// What a task graph is built for. Offsets always carry the symbolic stride PT_LD.
struct GraphSpec {
    int T, E;              // tiles of the block; tile columns right of it (wide panel)
    bool stream;           // XS tasks beside the leaves (GPX_PANEL_STREAM, the default)
    bool aug;              // E = 1 is a right-hand side of a WHOLE matrix
    int ig;                // tiles per inverse group (gpx_inverse_group; T: all of R^-1)
    bool sweep;            // the phases of a lock-step sweep: the fused spine task of round 2,
                           // no batched updates, no split, no fold
};

// the list of a panel launch: [ntasks] tasks of the general queue in schedule order, then
// [nspine] tasks of the spine
struct PanelTasks {
    std::vector<PTask> tasks;
    int ntasks = 0, nspine = 0, nctr = 0;
};
// solo (round 5): the list of a launch whose workgroups each run ONE member's whole graph, task
// after task in generation order (a topological order that also holds for the tasks whose data
// a follower polls: every producer has finished before its consumer starts) -- all tasks are
// "spine" tasks of a single spine workgroup per member, the queue is empty. solo = 2: without
// the tasks of the inverse (nothing reads W: value-only members).
int panel_tasks(const GraphSpec &spec, int workers, int solo, PanelTasks *out);

// the tasks of a lock-step sweep over T tiles [+ E = 1: a right-hand side], phase by phase
// (0 = F(0), 1 + s = X(s), fused task first), stripped of their counters
struct SweepTasks {
    std::vector<PTask> tasks;
    std::vector<int> first, count;
};
int sweep_tasks(int T, int E, SweepTasks *out);

int panel_kbatch(int T, int E);
bool panel_split(bool stream, int E, bool aug);
bool panel_fold();

bool gpx_panel_grid_fits(int nmem, int nspwg, int ncu);
bool panel_grid_members(int nmem, int ncu, bool whole, bool split, bool fold, int *nspwg,
                        int *workers);
bool panel_grid_single(int np, int T, int E, bool whole, bool split, int ncu, int *nspwg,
                       int *workers);
