// Tiled fp32 MFMA GEMM (gemm_tiled.hip) — interface for kernels.hip.
#pragma once
#include <ATen/ATen.h>
#include <c10/util/Optional.h>
#include <cstdint>

namespace bns {

// Operand layouts of the three project GEMMs. Every operand is a
// contiguous row-major matrix; R is the reduction length.
//   NT: C[M,N] = A[M,R] @ B[N,R]^T (+bias)   y  = x @ w^T + b
//   NN: C[M,N] = A[M,R] @ B[R,N]             dx = g @ w
//   TN: C[M,N] = A[R,M]^T @ B[R,N]           dw = g^T @ x
enum GemmLayout { GEMM_NT = 0, GEMM_NN = 1, GEMM_TN = 2 };

// Which operand gets dropout applied while it is staged (the mask index
// is the operand's flat element offset): the activation x is A in NT and
// B in TN.
enum GemmDrop { DROP_NONE = 0, DROP_A = 1, DROP_B = 2 };

// True when the float4 fast path applies: 16-byte-aligned bases and every
// operand's contiguous dimension divisible by 4.
bool gemm_tiled_aligned(GemmLayout layout, const at::Tensor& A,
                        const at::Tensor& B, int M, int N, int R);

// Runs the tiled kernel at ANY shape (unaligned operands take its scalar
// staging path); split-K with atomics into a zeroed C when the tile grid
// alone cannot fill the device. M, N, R > 0.
at::Tensor gemm_tiled(GemmLayout layout, const at::Tensor& A,
                      const at::Tensor& B,
                      const c10::optional<at::Tensor>& bias, int M, int N,
                      int R, GemmDrop drop = DROP_NONE, float keep = 1.0f,
                      uint64_t seed = 0);

}  // namespace bns
