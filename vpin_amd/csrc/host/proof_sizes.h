// proof_sizes.h -- how many bytes a computation commitment and a SNARK proof take, from an instance's dimensions alone.
// Plain arithmetic, no field, no device: the prover sizes its buffers with it (prover.cpp, spark.cpp) and the proof record's
// codec (wire_proof.cpp) bounds with it what a header from an untrusted peer can make a receiver allocate.
#pragma once
#include <algorithm>
#include <cstddef>

namespace vpin_sizes {

inline size_t ceil_log2(size_t n) { size_t l = 0; while (((size_t)1 << l) < n) l++; return l; }
inline size_t next_pow2(size_t n) { return (size_t)1 << ceil_log2(n); }

// the rows of comm_para / comm_input (32 bytes each) under a padded num_vars: the left half of the matrix view of the
// assignment's polynomial (dense_mlpoly.rs:193-218)
inline size_t vars_rows(size_t num_vars) { return (size_t)1 << (ceil_log2(num_vars) / 2); }

inline size_t sat_proof_max_bytes(size_t num_cons, size_t num_vars) {
  const size_t lx = ceil_log2(num_cons), ly = ceil_log2(2 * num_vars), ell = ceil_log2(num_vars);
  const size_t L = (size_t)1 << (ell / 2), lgR = ell - ell / 2;
  return 8 + 32 * L + (lx + ly) * 400 + 2048 + 64 * lgR;
}

// SNARK::encode's shape: the padded entry count N, the memory size M, and the variables of the three commitment views
// (SparseMatPolyCommitmentGens::new, sparse_mlpoly.rs:300-329, batch_size = 3)
struct SparkShape { size_t nx, ny, N, M, v_ops, v_mem, v_derefs; };
inline SparkShape spark_shape(size_t num_cons, size_t num_vars, const size_t nnz[3]) {
  SparkShape s;
  s.nx = ceil_log2(num_cons);
  s.ny = ceil_log2(2 * num_vars);
  s.N = 1;
  for (int m = 0; m < 3; m++) s.N = std::max(s.N, next_pow2(nnz[m]));  // get_num_nz_entries (sparse_mlpoly.rs:364)
  s.M = (size_t)1 << std::max(s.nx, s.ny);
  s.v_ops = ceil_log2(s.N) + 4;
  s.v_mem = std::max(s.nx, s.ny) + 1;
  s.v_derefs = ceil_log2(s.N) + 3;
  return s;
}

// bincode(R1CSCommitment): six u64 and the two row-commitment vectors
inline size_t spark_comm_bytes(size_t num_cons, size_t num_vars, const size_t nnz[3]) {
  const SparkShape s = spark_shape(num_cons, num_vars, nnz);
  return 8 * 6 + 8 + 32 * ((size_t)1 << (s.v_ops / 2)) + 8 + 32 * ((size_t)1 << (s.v_mem / 2));
}

inline size_t snark_proof_max_bytes(size_t num_cons, size_t num_vars, const size_t nnz[3]) {
  const SparkShape s = spark_shape(num_cons, num_vars, nnz);
  const size_t lgN = ceil_log2(s.N), lgM = ceil_log2(s.M);
  size_t b = sat_proof_max_bytes(num_cons, num_vars) + 96;
  b += 8 + 32 * ((size_t)1 << (s.v_derefs / 2)) + 64 * 32;
  b += lgN * (lgN * 104 + 64 + 24 * 32 + 64) + 18 * 32 + 64;
  b += lgM * (lgM * 104 + 64 + 8 * 32 + 64) + 64;
  b += 3 * (16 + 64 * 40 + 128 + 64) + 40 * 32 + 1024;
  return b;
}

// One operation of a gadget: constraints, variables and the entries it adds to A, B, C (point_mult.rs:61-325 at n = 128,
// point_addition.rs:67-153).  vpin_gadget_shape counts the entries by emitting an operation; these are the same numbers as
// literals, so that the record codec needs no field arithmetic (tests/test_proof_wire_model.py holds the two together)
constexpr size_t kMultOpCons = 27 * 128 + 8, kMultOpVars = 27 * 128 + 10, kAddOpCons = 10, kAddOpVars = 15;
constexpr size_t kMultOpNnz[3] = {5260, 4488, 3201}, kAddOpNnz[3] = {16, 14, 10};

// the padded dimensions Instance::new gives a gadget of n_ops operations (lib.rs:138-244), as vpin_gadget_shape
inline void gadget_dims(int is_mult, size_t n_ops, size_t* num_cons, size_t* num_vars, size_t nnz[3]) {
  const size_t cons = (is_mult ? kMultOpCons : kAddOpCons) * n_ops, vars = (is_mult ? kMultOpVars : kAddOpVars) * n_ops + 1;
  for (int m = 0; m < 3; m++) nnz[m] = (is_mult ? kMultOpNnz : kAddOpNnz)[m] * n_ops;
  *num_vars = next_pow2(vars);
  *num_cons = cons <= 1 ? 2 : next_pow2(cons);
}

}  // namespace vpin_sizes
