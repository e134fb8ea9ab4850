/* ref_glue_baij.c — TEST INFRASTRUCTURE.  Doors with plain arrays into the reference's PETSc-bound kernels
 * (src/kernels/*.c), compiled where they lie against oracle/petsc_stub (oracle/Makefile).  One file, three libraries:
 *   -DREF_GLUE_SOLVE  _ref/libref_baij_solve.so   MatSolve_SeqBAIJ_4, MatSolve_SeqBAIJ_4_AVX2
 *   -DREF_GLUE_MULT   _ref/libref_baij_mult.so    MatMult_SeqBAIJ_4_FMA / _AVX2, MatMatMult_SeqBAIJ_4_AVX2, MatMult_SeqAIJ_FMA
 *   -DREF_GLUE_MAD    _ref/libref_baij_mad.so     MatMult_SeqBAIJ_4, MatMult_SeqAIJ
 * Each door builds the Mat_SeqBAIJ / Mat_SeqAIJ, Vec and IS on its stack (identity permutations) and hands the kernel its
 * OWN 32-byte-aligned copies of everything the kernel touches: the AVX2 kernels use aligned loads and stores on a->a,
 * solve_work, x and t, so they fault on a buffer that is only 16-byte aligned (numpy's, malloc's).  Returns the kernel's
 * PetscErrorCode, or -1 when a copy could not be allocated. */
#include "kernels.h"

static void *aligned_copy(const void *src, size_t bytes) {
  size_t padded = (bytes + 63) / 32 * 32; /* never zero; a multiple of the alignment, as aligned_alloc asks */
  void *p = aligned_alloc(32, padded);
  if (!p) return NULL;
  memset(p, 0, padded);
  if (src && bytes) memcpy(p, src, bytes);
  return p;
}

/* the compressed-row view PETSc keeps for a matrix with many empty rows: the nonempty block rows only */
typedef struct { Mat_SeqBAIJ a; struct _p_Mat mat; PetscInt *ci, *ridx; MatScalar *aa; } glue_baij;

static int glue_baij_init(glue_baij *g, int mbs, const int *ai, const int *aj, const double *aa, int compressed) {
  memset(g, 0, sizeof(*g));
  int nz = ai[mbs];
  g->aa = (MatScalar *)aligned_copy(aa, (size_t)nz * 16 * sizeof(double));
  g->ci = (PetscInt *)malloc(((size_t)mbs + 1) * sizeof(PetscInt));
  g->ridx = (PetscInt *)malloc(((size_t)mbs + 1) * sizeof(PetscInt));
  if (!g->aa || !g->ci || !g->ridx) return -1;
  int nrows = 0;
  g->ci[0] = 0;
  for (int i = 0; i < mbs; i++)
    if (ai[i + 1] > ai[i]) {
      g->ridx[nrows] = i;
      g->ci[++nrows] = ai[i + 1];
    }
  g->a.mbs = g->a.nbs = mbs;
  g->a.bs2 = 16;
  g->a.nz = nz;
  g->a.nonzerorowcnt = 4 * nrows;
  g->a.i = (PetscInt *)ai;
  g->a.j = (PetscInt *)aj;
  g->a.a = g->aa;
  g->a.compressedrow.use = compressed ? PETSC_TRUE : PETSC_FALSE;
  g->a.compressedrow.nrows = nrows;
  g->a.compressedrow.i = g->ci;
  g->a.compressedrow.rindex = g->ridx;
  g->mat.data = &g->a;
  return 0;
}

static void glue_baij_free(glue_baij *g) {
  free(g->aa);
  free(g->ci);
  free(g->ridx);
}

#if defined(REF_GLUE_MULT) || defined(REF_GLUE_MAD)
/* y = A x through one of the reference's BAIJ-4 products; aa: column-major blocks, as Mat_SeqBAIJ::a holds them */
static int baij_mult(PetscErrorCode (*fn)(Mat, Vec, Vec), int mbs, int nbcols, const int *ai, const int *aj, const double *aa,
                     const double *x, double *y, int compressed) {
  glue_baij g;
  int rc = -1;
  double *xc = NULL, *yc = NULL;
  if (glue_baij_init(&g, mbs, ai, aj, aa, compressed) == 0) {
    xc = (double *)aligned_copy(x, (size_t)nbcols * 4 * sizeof(double));
    yc = (double *)aligned_copy(NULL, (size_t)mbs * 4 * sizeof(double));
    if (xc && yc) {
      struct _p_Vec vx = {xc, 4 * nbcols}, vy = {yc, 4 * mbs};
      rc = fn(&g.mat, &vx, &vy);
      memcpy(y, yc, (size_t)mbs * 4 * sizeof(double));
    }
  }
  free(xc);
  free(yc);
  glue_baij_free(&g);
  return rc;
}

static int aij_mult(PetscErrorCode (*fn)(Mat, Vec, Vec), int n, int ncols, const int *ai, const int *aj, const double *aa, const double *x,
                    double *y) {
  Mat_SeqAIJ a;
  struct _p_Mat mat;
  struct _p_PetscLayout rmap = {n}, cmap = {ncols};
  memset(&a, 0, sizeof(a));
  memset(&mat, 0, sizeof(mat));
  a.nz = ai[n];
  a.i = (PetscInt *)ai;
  a.j = (PetscInt *)aj;
  a.a = (MatScalar *)aa;
  mat.data = &a;
  mat.rmap = &rmap;
  mat.cmap = &cmap;
  struct _p_Vec vx = {(double *)x, ncols}, vy = {y, n};
  return fn(&mat, &vx, &vy);
}
#endif

#ifdef REF_GLUE_SOLVE
/* x = U^-1 L^-1 b on PETSc's factored BAIJ layout (tests/petsc_layout.py): kind 0 MatSolve_SeqBAIJ_4, 1 ..._AVX2.
 * inplace: the kernel is handed ONE vector as both b and x, as a caller that solves in place does. */
int ref_baij_solve(int kind, int mbs, const int *bi, const int *bj, const int *bdiag, const double *ba, int nblocks, const double *b,
                   double *x, int inplace) {
  if (mbs <= 0) return 0; /* the scalar kernel reads r[0] and b[0..3] before it looks at n */
  int rc = -1;
  PetscInt *ident = (PetscInt *)malloc((size_t)mbs * sizeof(PetscInt));
  double *aa = (double *)aligned_copy(ba, (size_t)nblocks * 16 * sizeof(double));
  double *work = (double *)aligned_copy(NULL, (size_t)mbs * 4 * sizeof(double));
  double *bc = (double *)aligned_copy(b, (size_t)mbs * 4 * sizeof(double));
  double *xc = inplace ? bc : (double *)aligned_copy(NULL, (size_t)mbs * 4 * sizeof(double));
  if (ident && aa && work && bc && xc) {
    for (int i = 0; i < mbs; i++) ident[i] = i;
    struct _p_IS is = {ident};
    Mat_SeqBAIJ a;
    struct _p_Mat mat;
    struct _p_PetscLayout map = {4 * mbs};
    memset(&a, 0, sizeof(a));
    memset(&mat, 0, sizeof(mat));
    a.mbs = a.nbs = mbs;
    a.bs2 = 16;
    a.nz = nblocks;
    a.i = (PetscInt *)bi;
    a.j = (PetscInt *)bj;
    a.diag = (PetscInt *)bdiag;
    a.a = aa;
    a.row = a.col = a.icol = &is;
    a.solve_work = work;
    a.pivotinblocks = PETSC_TRUE;
    mat.data = &a;
    mat.rmap = mat.cmap = &map;
    struct _p_Vec vb = {bc, 4 * mbs}, vx = {xc, 4 * mbs};
    rc = kind == 0 ? MatSolve_SeqBAIJ_4(&mat, inplace ? &vx : &vb, &vx) : MatSolve_SeqBAIJ_4_AVX2(&mat, inplace ? &vx : &vb, &vx);
    memcpy(x, xc, (size_t)mbs * 4 * sizeof(double));
  }
  free(ident);
  free(aa);
  free(work);
  free(bc);
  if (!inplace) free(xc);
  return rc;
}
#endif

#ifdef REF_GLUE_MULT
/* kind 1 MatMult_SeqBAIJ_4_FMA, 2 MatMult_SeqBAIJ_4_AVX2 */
int ref_baij_mult(int kind, int mbs, int nbcols, const int *ai, const int *aj, const double *aa, const double *x, double *y, int compressed) {
  if (kind != 1 && kind != 2) return -2;
  return baij_mult(kind == 1 ? MatMult_SeqBAIJ_4_FMA : MatMult_SeqBAIJ_4_AVX2, mbs, nbcols, ai, aj, aa, x, y, compressed);
}

/* kind 1 MatMult_SeqAIJ_FMA */
int ref_aij_mult(int kind, int n, int ncols, const int *ai, const int *aj, const double *aa, const double *x, double *y) {
  if (kind != 1) return -2;
  return aij_mult(MatMult_SeqAIJ_FMA, n, ncols, ai, aj, aa, x, y);
}

/* Y = MatMatMult_SeqBAIJ_4_AVX2(A, X, s): X and Y are 4 mbs x s, column-major with leading dimension 4 mbs (the kernel's lda),
 * so the matrix must be square.  aa goes to the kernel byte for byte: which bytes make it compute A X is the caller's business. */
int ref_baij_spmm(int mbs, const int *ai, const int *aj, const double *aa, const double *X, double *Y, int s, int compressed) {
  glue_baij g;
  int rc = -1;
  double *xc = NULL, *yc = NULL;
  size_t len = (size_t)mbs * 4 * (size_t)s;
  if (glue_baij_init(&g, mbs, ai, aj, aa, compressed) == 0) {
    xc = (double *)aligned_copy(X, len * sizeof(double));
    yc = (double *)aligned_copy(NULL, len * sizeof(double));
    if (xc && yc) {
      struct _p_Mat mx, my;
      memset(&mx, 0, sizeof(mx));
      memset(&my, 0, sizeof(my));
      mx.dense = xc;
      my.dense = yc;
      rc = MatMatMult_SeqBAIJ_4_AVX2(&g.mat, &mx, &my, s);
      memcpy(Y, yc, len * sizeof(double));
    }
  }
  free(xc);
  free(yc);
  glue_baij_free(&g);
  return rc;
}
#endif

#ifdef REF_GLUE_MAD
/* kind 0 MatMult_SeqBAIJ_4 */
int ref_baij_mult(int kind, int mbs, int nbcols, const int *ai, const int *aj, const double *aa, const double *x, double *y, int compressed) {
  if (kind != 0) return -2;
  return baij_mult(MatMult_SeqBAIJ_4, mbs, nbcols, ai, aj, aa, x, y, compressed);
}

/* kind 0 MatMult_SeqAIJ */
int ref_aij_mult(int kind, int n, int ncols, const int *ai, const int *aj, const double *aa, const double *x, double *y) {
  if (kind != 0) return -2;
  return aij_mult(MatMult_SeqAIJ, n, ncols, ai, aj, aa, x, y);
}
#endif
