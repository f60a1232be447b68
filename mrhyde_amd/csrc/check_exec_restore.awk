# check_exec_restore.awk -- reads a kernel file's device assembly; fails when a basic block holds a register-to-register
# copy or scratch traffic between its label and the `s_or_b64 exec, exec, ...` that restores the exec mask behind a
# divergent region.  Such an instruction runs for the lanes that are still active there -- none behind a loop with a
# divergent exit -- so the value it was to carry over is lost for the others.  The compiler placed copies and spills of
# values live across the dof-gather loop there in five 3-D deck-string builds of jacobian_diagonal_kernel (the diagonal
# came out 0.0 or stale); see the kernel's note on `wave`.
/^_ZN.*:/ { fn = $1 }
/^\.LBB[0-9_]+:/ { open = 1; n = 0; label = $1; next }
open && /^[ \t]+s_or_b64 exec, exec,/ {
  if (n) { printf "%s %s %d instruction(s) before the exec restore, first:%s\n", fn, label, n, first; bad++ }
  open = 0; next
}
open && /^[ \t]+(v_mov_b32_e32 v[0-9]+, v[0-9]+$|v_mov_b64_e32 v\[[0-9:]+\], v\[|v_accvgpr|scratch_[ls])/ {   # (vector copies, AGPR moves, private-memory loads and stores)
  if (!n) first = $0
  n++; next
}
open && /^[ \t]+(s_cbranch|s_branch|s_andn2_b64 exec|s_and_saveexec|s_mov_b64 exec)/ { open = 0; next }
END { if (bad) { print bad " block(s) copy or spill before the exec mask is restored: refusing to build"; exit 1 } }
