/* forwards to the hand-written stand-in for PETSc (petsc_stub.h); see there */
#include <petsc_stub.h>
