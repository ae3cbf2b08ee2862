# usymlqr.jl -- usymlqr! through the specialised method (the library's device-resident loop on A and A') against the generic method
# of Krylov.jl on the same device types.  It does its own set-up: run it stand-alone, or include it after runtests.jl:
#
#   julia --project=julia/KrylovHIP julia/KrylovHIP/test/usymlqr.jl     (needs an MI355X and krylov.jl_amd/libkrylov_hip.so)
using Test, LinearAlgebra, SparseArrays
using Krylov, KrylovHIP
import KrylovHIP: HIPVector, HIPCsr, CTX, Ctx

@isdefined(kron_unsymmetric) || include(joinpath(pkgdir(Krylov), "test", "test_utils.jl"))   # kron_unsymmetric, small_sqd, ...

if !@isdefined(native)                                               # stand-alone: runtests.jl has made the context and `native`
  CTX[] = Ctx(0)
  function native(body, path::Integer)
    n0 = KrylovHIP.NATIVE_SOLVES[]; g0 = KrylovHIP.GENERIC_SOLVES[]
    out = body()
    @test KrylovHIP.NATIVE_SOLVES[] == n0 + 1
    @test KrylovHIP.GENERIC_SOLVES[] == g0
    @test KrylovHIP.LAST_PATH[] == path
    out
  end
end
generic(f!, ws, A, b, c; kw...) = invoke(f!, Tuple{typeof(ws),Any,AbstractVector{Float64},AbstractVector{Float64}}, ws, A, b, c; kw...)
saddle_residual(A, b, c, x, y) = norm([b - x - A * y; c - A' * x]) / norm([b; c])

@testset "usymlqr! -- KrylovHIP" begin
  A_cpu, b_cpu = kron_unsymmetric(7)
  A_cpu = sparse(A_cpu) + 24.0 * I
  n = size(A_cpu, 1)
  c_cpu = sin.(0.11 .* (0:n-1)) .+ 1.2
  A_gpu = HIPCsr(A_cpu)
  b = HIPVector(b_cpu)
  c = HIPVector(c_cpu)
  S = HIPVector

  @testset "usymlqr(A_gpu, b_gpu, c_gpu)" begin
    x, y, stats = native(2) do; usymlqr(A_gpu, b, c); end            # forwards callback = workspace -> false
    @test stats.solved && !stats.inconsistent
    @test saddle_residual(A_cpu, b_cpu, c_cpu, Vector(x), Vector(y)) ≤ 1e-6
    @test A_gpu' === A_gpu'                                          # A' is built once and kept on the matrix
  end

  @testset "native against generic" begin
    ws = UsymlqrWorkspace(n, n, S, S); ws2 = UsymlqrWorkspace(n, n, S, S)
    native(2) do; usymlqr!(ws, A_gpu, b, c; history = true); end
    generic(usymlqr!, ws2, A_gpu, b, c; history = true)
    @test ws.stats.niter == ws2.stats.niter
    @test ws.stats.status == ws2.stats.status == "solution good enough given atol and rtol"
    @test length(ws.stats.residuals) == length(ws2.stats.residuals)  # per iteration: the least-squares entry, then the least-norm entry
    @test ws.stats.residuals ≈ ws2.stats.residuals rtol = 1e-5
    @test length(ws.stats.Aresiduals) == length(ws2.stats.Aresiduals)
    @test ws.stats.Aresiduals ≈ ws2.stats.Aresiduals rtol = 1e-5
    @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
    @test Vector(ws.y) ≈ Vector(ws2.y) rtol = 1e-6
    for kw in ((itmax = 1,), (itmax = 2,), (itmax = 3,), (itmax = 4,), (itmax = 7,), (ls = false,), (ln = false,), (rtol = 1e-3,))
      native(2) do; usymlqr!(ws, A_gpu, b, c; kw...); end
      generic(usymlqr!, ws2, A_gpu, b, c; kw...)
      @test ws.stats.niter == ws2.stats.niter
      @test ws.stats.status == ws2.stats.status
      @test (ws.stats.solved, ws.stats.inconsistent) == (ws2.stats.solved, false)
      @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6 atol = 1e-6 * norm(b_cpu)
      @test Vector(ws.y) ≈ Vector(ws2.y) rtol = 1e-6
    end
    @test_throws Exception usymlqr!(ws, A_gpu, b, c; ls = false, ln = false)
  end

  @testset "warm start, callback, verbose" begin
    ws = UsymlqrWorkspace(n, n, S, S)
    x0 = HIPVector(collect(range(-0.5, 0.5; length = n)))
    y0 = HIPVector(collect(range(0.25, -0.25; length = n)))
    native(2) do; usymlqr!(ws, A_gpu, b, c, x0, y0); end
    @test ws.stats.solved && saddle_residual(A_cpu, b_cpu, c_cpu, Vector(ws.x), Vector(ws.y)) ≤ 1e-6
    seen = Int[]
    native(1) do
      usymlqr!(ws, A_gpu, b, c; history = true, callback = w -> (push!(seen, length(w.stats.residuals)); length(seen) == 3))
    end
    @test seen == [2, 4, 6]                                          # nothing is pushed before iteration 1; two entries per iteration
    @test ws.stats.status == "user-requested exit"
    io = IOBuffer()                                                  # no file descriptor: the generic method prints
    g0 = KrylovHIP.GENERIC_SOLVES[]
    usymlqr!(ws, A_gpu, b, c; verbose = 1, iostream = io)
    @test KrylovHIP.GENERIC_SOLVES[] == g0 + 1
    @test occursin("USYMLQR: system of $(2n) equations in $(2n) variables", String(take!(io)))
  end

  @testset "rectangular systems" begin
    for transpose in (false, true)
      Ar, br, cr, _, _ = small_sqd(transpose)
      mr, nr = size(Ar)
      mr > nr || continue                                            # full column rank: the least-squares problem is well posed
      ws = UsymlqrWorkspace(mr, nr, S, S); ws2 = UsymlqrWorkspace(mr, nr, S, S)
      native(0) do; usymlqr!(ws, HIPCsr(sparse(Ar)), HIPVector(br), HIPVector(cr); itmax = nr); end   # m ≠ n: the primitive sequence
      generic(usymlqr!, ws2, HIPCsr(sparse(Ar)), HIPVector(br), HIPVector(cr); itmax = nr)
      @test length(ws.x) == mr && length(ws.y) == nr
      @test ws.stats.niter == ws2.stats.niter
      @test Vector(ws.x) ≈ Vector(ws2.x) rtol = 1e-6
      @test Vector(ws.y) ≈ Vector(ws2.y) rtol = 1e-6
    end
  end
end
