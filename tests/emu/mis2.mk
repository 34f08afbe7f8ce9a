# TEST INFRASTRUCTURE: the emulator library of Makefile plus the MIS-2 / aggregation / coarsening unit (kk_mis2.hip), for
# tests/test_emu_mis2.py.  Makefile itself stays as it is; its objects are shared.
include Makefile
libkkamd_emu_mis2.so: $(OBJS) kk_mis2.emu.o
	$(CXX) -shared -o $@ $(OBJS) kk_mis2.emu.o
