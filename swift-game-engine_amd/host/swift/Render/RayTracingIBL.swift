//  RayTracingIBL.swift — IBLResources (Game/IBLResources.swift) and the envMap / brdfLUT side of RayTracingRenderer
//  (RayTracingRenderer.swift:86, :141) over include/sge_amd_render_ibl.h. NOT COMPILED HERE (see ../GPUCrowd.swift). C++ twin:
//  sge::IBLResources and sge::RayTracingRenderer::setIBL / clearIBL in ../../sge_host.hpp.
//
//  The cube is rgba16Float as halves (UInt16 bits), level-major, then face +X -X +Y -Y +Z -Z, then rows; the table is rgba32Float.
//  Specular IBL is active while both are set.

import CSGE
import CSGERender

public final class IBLResources {
    public let envCube: [UInt16]
    public let brdfLUT: [Float]
    public let envSize: Int
    public let envMipCount: UInt32
    public let lutSize: Int

    /// IBLResources.init: the procedural cube at 128 with its full chain, the 128 x 128 table with 256 samples
    public convenience init() { self.init(envSize: 128, lutSize: 128, sampleCount: 256) }

    public init(envSize: Int, lutSize: Int, sampleCount: Int) {
        var mips = 1
        var s = envSize
        while s > 1 { s >>= 1; mips += 1 }
        var texels = 0
        for m in 0..<mips { let n = max(envSize >> m, 1); texels += 6 * n * n }
        var cube = [UInt16](repeating: 0, count: max(texels, 1) * 4)
        precondition(sge_ibl_default_env_build(Int32(envSize), Int32(mips), &cube) == SGE_OK)
        var lut = [Float](repeating: 0, count: max(lutSize * lutSize, 1) * 4)
        precondition(sge_ibl_default_brdf_lut_build(Int32(lutSize), Int32(sampleCount), &lut) == SGE_OK)
        self.envCube = cube
        self.brdfLUT = lut
        self.envSize = envSize
        self.envMipCount = UInt32(mips)
        self.lutSize = lutSize
    }
}

public final class RayTracingIBL {
    private let crowd: GPUCrowd
    public init?(crowd: GPUCrowd?) {
        guard let crowd = crowd else { return nil }
        self.crowd = crowd
    }

    /// the envMap and brdfLUT bindings, and frame.envMipCount
    public func setIBL(_ ibl: IBLResources) {
        precondition(ibl.envSize <= Int(SGE_MAX_ENV_SIZE) && ibl.envMipCount <= UInt32(SGE_MAX_ENV_MIPS) && ibl.lutSize <= Int(SGE_MAX_BRDF_LUT_DIM))
        crowd.check(sge_render_env_upload(crowd.ctx, Int32(ibl.envSize), Int32(ibl.envMipCount), ibl.envCube))
        crowd.check(sge_render_brdf_lut_upload(crowd.ctx, Int32(ibl.lutSize), Int32(ibl.lutSize), ibl.brdfLUT))
    }

    public func clearIBL() {
        crowd.check(sge_render_ibl_clear(crowd.ctx))
    }

    /// nil fields for an empty resource
    public func info() -> (envSize: Int, envMipCount: Int, lutWidth: Int, lutHeight: Int) {
        var s: Int32 = 0, m: Int32 = 0, w: Int32 = 0, h: Int32 = 0
        crowd.check(sge_render_ibl_info_get(crowd.ctx, &s, &m, &w, &h))
        return (Int(s), Int(m), Int(w), Int(h))
    }

    /// the frame kernels' cube sampler alone: rgb per direction and level of detail
    public func sampleEnvironment(dirs: [Float], lods: [Float]) -> [Float] {
        var out = [Float](repeating: 0, count: lods.count * 3)
        crowd.check(sge_render_env_sample_batch(crowd.ctx, dirs, lods, Int32(lods.count), &out))
        return out
    }

    /// the table sampler alone: x and y per uv pair
    public func sampleBrdfLUT(uvs: [Float]) -> [Float] {
        var out = [Float](repeating: 0, count: uvs.count)
        crowd.check(sge_render_brdf_lut_sample_batch(crowd.ctx, uvs, Int32(uvs.count / 2), &out))
        return out
    }

    /// the same over device memory, enqueued on the context's stream
    public func sampleEnvironment(deviceDirs: UnsafeRawPointer, deviceLods: UnsafeRawPointer, count: Int, deviceRGB: UnsafeMutableRawPointer) {
        crowd.check(sge_render_env_sample_device(crowd.ctx, deviceDirs, deviceLods, Int32(count), deviceRGB))
    }

    public func sampleBrdfLUT(deviceUVs: UnsafeRawPointer, count: Int, deviceOut: UnsafeMutableRawPointer) {
        crowd.check(sge_render_brdf_lut_sample_device(crowd.ctx, deviceUVs, Int32(count), deviceOut))
    }
}
