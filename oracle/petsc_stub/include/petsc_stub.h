/* petsc_stub.h — TEST INFRASTRUCTURE.  The few PETSc names that the reference's solver kernels (src/kernels/*.c) touch,
 * declared by hand from the way those files use them, so that they compile where they lie without PETSc (oracle/Makefile,
 * targets _ref/libref_baij_*.so).  Nothing here does what PETSc does: a Vec is a pointer to doubles, an IS a pointer to
 * indices, a Mat a pointer to its implementation struct, and every call without an effect on the arithmetic (logging,
 * printing, Restore*) is inert.  oracle/ref_glue_baij.c fills the structs. */
#ifndef PETSC_STUB_H
#define PETSC_STUB_H

#include <stddef.h>
#include <stdlib.h>
#include <string.h>

typedef int PetscErrorCode;
typedef int PetscInt; /* the arrays of every handle of this project are 32-bit, as a default PETSc build's are */
typedef double PetscScalar;
typedef double MatScalar;
typedef double PetscReal;
typedef double PetscLogDouble;
typedef int PetscBool;
#define PETSC_TRUE 1
#define PETSC_FALSE 0
#define PETSC_SUCCESS 0
#define PETSC_ERR_ARG_OUTOFRANGE 63
#define PETSC_ERR_ARG_CORRUPT 64
#define PETSC_ERR_ARG_NULL 85
#define PETSC_COMM_SELF 0
#define PETSC_COMM_WORLD 0
#define PETSC_DECIDE (-1)

typedef struct _p_PetscLayout { PetscInt n; } *PetscLayout;
typedef struct _p_Vec { PetscScalar *array; PetscInt n; } *Vec;
typedef struct _p_IS { const PetscInt *idx; } *IS;
typedef struct _p_Mat { void *data; PetscLayout rmap, cmap; PetscScalar *dense; } *Mat; /* dense: the array of a MATDENSE */
typedef struct _p_KSP *KSP;
typedef struct { PetscReal fill; } MatFactorInfo;

typedef struct { PetscBool use; PetscInt nrows; PetscInt *i; PetscInt *rindex; } Mat_CompressedRow;
typedef struct {
  PetscInt mbs, nbs, bs2, nz, nonzerorowcnt;
  PetscInt *i, *j, *diag;
  MatScalar *a;
  IS row, col, icol;
  PetscScalar *solve_work;
  PetscBool pivotinblocks;
  Mat_CompressedRow compressedrow;
} Mat_SeqBAIJ;
typedef struct {
  PetscInt nz;
  PetscInt *i, *j, *diag;
  MatScalar *a;
} Mat_SeqAIJ;

#define PetscFunctionBegin do { } while (0)
#define PetscFunctionReturn(x) return (x)
#define PetscCall(...) do { PetscErrorCode petsc_stub_ierr_ = (__VA_ARGS__); if (petsc_stub_ierr_) return petsc_stub_ierr_; } while (0)
#define PetscCheck(cond, comm, err, ...) do { if (!(cond)) return (err); } while (0)
#define PetscMin(a, b) (((a) < (b)) ? (a) : (b))
#define PetscMax(a, b) (((a) < (b)) ? (b) : (a))
#define PetscLogFlops(x) PETSC_SUCCESS
#define PetscPrintf(...) PETSC_SUCCESS
#define PetscArrayzero(p, n) (memset((p), 0, (size_t)(n) * sizeof(*(p))), PETSC_SUCCESS)
#define PetscArraycpy(d, s, n) (memcpy((d), (s), (size_t)(n) * sizeof(*(d))), PETSC_SUCCESS)
#define PetscMalloc1(n, p) ((*(p) = malloc((size_t)(n) * sizeof(**(p)))) ? PETSC_SUCCESS : 55)
#define PetscFree(p) (free(p), (p) = NULL, PETSC_SUCCESS)

#define VecGetArray(v, p) (*(p) = (v)->array, PETSC_SUCCESS)
#define VecGetArrayRead(v, p) (*(p) = (v)->array, PETSC_SUCCESS)
#define VecGetArrayWrite(v, p) (*(p) = (v)->array, PETSC_SUCCESS)
#define VecRestoreArray(v, p) PETSC_SUCCESS
#define VecRestoreArrayRead(v, p) PETSC_SUCCESS
#define VecRestoreArrayWrite(v, p) PETSC_SUCCESS
#define ISGetIndices(is, p) (*(p) = (is)->idx, PETSC_SUCCESS)
#define ISRestoreIndices(is, p) PETSC_SUCCESS
#define MatDenseGetArray(m, p) (*(p) = (m)->dense, PETSC_SUCCESS)
#define MatDenseGetArrayRead(m, p) (*(p) = (m)->dense, PETSC_SUCCESS)
#define MatDenseRestoreArray(m, p) PETSC_SUCCESS
#define MatDenseRestoreArrayRead(m, p) PETSC_SUCCESS

/* named only by BuildKrylovBasis_AVX2 (spmm_avx2.c), which nothing here calls: they compile and do nothing */
#define KSPGetOperators(...) PETSC_SUCCESS
#define VecGetSize(...) PETSC_SUCCESS
#define MatCreateDense(...) PETSC_SUCCESS
#define MatDenseGetColumn(...) PETSC_SUCCESS
#define MatDenseRestoreColumn(...) PETSC_SUCCESS
#define MatDestroy(...) PETSC_SUCCESS
#define VecCopy(...) PETSC_SUCCESS
#define VecPlaceArray(...) PETSC_SUCCESS
#define VecResetArray(...) PETSC_SUCCESS

#endif
