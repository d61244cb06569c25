/* TEST INFRASTRUCTURE ONLY: the reference's two public headers in one, the
 * input of the precompiled header oracle/_ref/ref_api.h.gch that
 * oracle/build_ref.sh makes where the reference is present
 * (tests/test_abi.py::test_reference_header_and_ours_agree includes it
 * before ours, so every prototype both declare must be compatible). */
#include <shmem.h>
#include <pshmem.h>
