#pragma once
// run-time tuning switches (api.hip); initial values from the environment, changeable through gode_set_option
int gode_opt_gemm_split();   // GODE_GEMM_SPLIT (default 2): split-bf16 forward dense product at d = 128 - 1 always, 2 launches of <= 2 terms and >= 65 536 rows, 0 never
int gode_opt_overlap();      // GODE_OVERLAP (default 1): two-stream schedule of the adjoint rk4 driver
int gode_opt_wgrad_split();  // GODE_WGRAD_SPLIT (default 8): weight gradient at d = 128 from exact bf16 pieces with 8 (or 6) piece products per product; 0 = fp32-MFMA kernel
int gode_opt_wgrad_split_small();  // wgrad_split_small (default 0): use it below 65 536 rows too (tests)
int gode_opt_bwd_pc();       // GODE_BWD_PC (default 1): VJP at d = 128, >= 65 536 rows in producer / consumer form on the bf16 matrix cores (gemm_pc.hip)
int gode_opt_fwd_pc();       // GODE_FWD_PC (default 3): forward product likewise; bit 0 = launches of <= 2 terms, bit 1 = launches of >= 3 terms or with x_out
int gode_opt_small_fused();   // GODE_SMALL_FUSED (default 1): launch-bound graphs take the fused one-launch f-eval / VJP of csrc/small.hip
int gode_opt_bwd_wgrad();     // GODE_BWD_WGRAD (default 1): VJP and weight gradient of the ODE function at d = 128, >= 65 536 rows in ONE pass (gemm_pc.hip: gn_gemm_bwd_wgrad_pc_kernel) where the drivers issue both
int gode_opt_y2_colsum();     // GODE_Y2_COLSUM (default 1): the adjoint rk4 driver reduces a stage's bias gradient from the per-block column sums its forward-recompute SpMM leaves (workspace y2_colsum) instead of from dZ
int gode_opt_rk_close_once(); // GODE_RK_CLOSE_ONCE (default 1): the rk4 drivers above 65 536 rows at d = 128 form a step's closing combination y + h sum b_j k_j once, in the launch that already holds its four terms (last stage's dense product / SpMM), and the closing launch reads that one array
int gode_opt_spmm_pipe();     // GODE_SPMM_PIPE (default 1): the thread-group SpMM (> 65 536 records) without a cotangent output walks several tiles of records per block, the records' indices fetched ahead (spmm.hip: spmm_vec4_pipe_kernel), same bits; 0 = one tile per block (spmm_vec4_kernel); 2..64 = that many tiles per block (measurements and tests)
int gode_opt_diag_rows();     // GODE_DIAG_ROWS (default 1): where the ODE function carries the core record lists (gode_gcn_odefunc_t: a_core_items / a_diag, at_core_items / at_diag), the rk4 drivers above 65 536 rows take the rows that hold their diagonal only out of SpMM launches - forward solve, stages 0-2: the dense launch stores relu(a_ii S[i] + b) itself; adjoint solve, one-pass branch: Sp(g) stores a_ii dZ[i] of an isolated row straight into dS; same bits; 0 = the full lists
