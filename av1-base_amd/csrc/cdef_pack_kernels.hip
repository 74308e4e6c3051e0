// cdef_pack_kernels.hip - the former name of the file that held CDEF and the packing kernels together.  CDEF is cdef_kernel.hip now
// and the packing and SSE kernels are pack_kernels.hip; this name stays for translation units that include the packing kernels by it
// (the launch harness of tests/test_entropy_kernels.py did, and the suite of an earlier revision still does when it is run on this
// tree).  Not a source of the library: build.py does not list it.
#include "pack_kernels.hip"
