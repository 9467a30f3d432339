#!/bin/bash
# Diagnostic: dp_temporal_kernel with phase stamps (-DDPT_STAMPS) -> _scratch/lib_tstamps.so (other objects: the product build's);
# tools/temporal_phases.py then prints where one launch's cycles go.  Build on the build host, run the .py on the GPU box.
set -e
mkdir -p _scratch
B=dragposer_amd/csrc/_build
FLAGS=$(python3 -c "import __graft_entry__ as g; print(' '.join(f for f in g.HIPCC_FLAGS if f != '-shared'))")
hipcc $FLAGS -DDPT_STAMPS $EXTRA -c dragposer_amd/csrc/dp_temporal.hip -o _scratch/dp_temporal_stamps.o
# every other object of the product as build() left it (the predictor's host side, dp_temporal_host.o, among them)
OBJS=$(python3 -c "import __graft_entry__ as g, os; print(' '.join('$B/' + os.path.splitext(s)[0] + '.o' for s in g.HIP_SOURCES if s != 'dp_temporal.hip'))")
hipcc --offload-arch=gfx950 -shared -fPIC -o _scratch/lib_tstamps.so $OBJS _scratch/dp_temporal_stamps.o
echo _scratch/lib_tstamps.so
