//  RayTracingTextures.swift — the texture side of RayTracingRenderer (TextureResource.swift, RTGeometryCache.swift:328-353) over
//  include/sge_amd_render_textures.h. NOT COMPILED HERE (see ../GPUCrowd.swift). C++ twin: the texture calls of
//  sge::RayTracingRenderer in ../../sge_host.hpp.
//
//  A texture is one of the 32 slots of the kernel's texture array; a material's texture indices name slots. A slot that holds no
//  texture is what `index >= textureCount` is in the Metal text: the material behaves as if it named none.

import CSGE
import CSGERender

/// RTInstanceInfo's texture indices (ShaderTypes.h:118-124) and Material.normalScale (Material.swift:46); nil = no texture
public struct RTMaterialTextures {
    public var baseColor: Int?, normal: Int?, metallicRoughness: Int?, emissive: Int?, occlusion: Int?
    public var normalScale: Float = 1
    public init() {}
    var record: sge_render_material_textures {
        sge_render_material_textures(baseColor: Int32(baseColor ?? -1), normal: Int32(normal ?? -1), metallicRoughness: Int32(metallicRoughness ?? -1),
                                     emissive: Int32(emissive ?? -1), occlusion: Int32(occlusion ?? -1), normalScale: normalScale, pad: (0, 0))
    }
}

public final class RayTracingTextures {
    private let crowd: GPUCrowd
    public init?(crowd: GPUCrowd?) {
        guard let crowd = crowd else { return nil }
        self.crowd = crowd
    }

    /// texture.replace(region:mipmapLevel:withBytes:bytesPerRow:) with bytesPerRow = width * 4: rgba8Unorm, or rgba8Unorm_srgb
    public func replace(slot: Int, width: Int, height: Int, srgb: Bool, rgba: [UInt8]) {
        precondition(rgba.count == width * height * 4)
        crowd.check(sge_render_texture_upload(crowd.ctx, Int32(slot), Int32(width), Int32(height),
                                              srgb ? Int32(SGE_TEX_RGBA8_UNORM_SRGB) : Int32(SGE_TEX_RGBA8_UNORM), rgba))
    }

    /// nil: every slot
    public func clear(slot: Int? = nil) {
        crowd.check(sge_render_texture_clear(crowd.ctx, Int32(slot ?? -1)))
    }

    /// entries for materials 0 ..< table.count; every other material returns to no textures
    public func setMaterialTextures(_ table: [RTMaterialTextures]) {
        let records = table.map { $0.record }
        crowd.check(sge_render_material_textures_set(crowd.ctx, Int32(records.count), records))
    }

    /// nil for an empty slot
    public func info(slot: Int) -> (width: Int, height: Int, srgb: Bool)? {
        var w: Int32 = 0, h: Int32 = 0, f: Int32 = 0
        crowd.check(sge_render_texture_info_get(crowd.ctx, Int32(slot), &w, &h, &f))
        return w == 0 ? nil : (Int(w), Int(h), f == Int32(SGE_TEX_RGBA8_UNORM_SRGB))
    }

    /// the 256 entries the kernels decode an rgba8Unorm_srgb colour channel with
    public func srgbTable() -> [Float] {
        var t = [Float](repeating: 0, count: 256)
        crowd.check(sge_render_srgb_table_get(crowd.ctx, &t))
        return t
    }

    /// the frame kernels' sampler alone: rgba per uv pair
    public func sample(slot: Int, uvs: [Float]) -> [Float] {
        var out = [Float](repeating: 0, count: uvs.count * 2)
        crowd.check(sge_render_texture_sample_batch(crowd.ctx, Int32(slot), uvs, Int32(uvs.count / 2), &out))
        return out
    }

    /// the same over device memory, enqueued on the context's stream
    public func sample(slot: Int, deviceUVs: UnsafeRawPointer, count: Int, deviceRGBA: UnsafeMutableRawPointer) {
        crowd.check(sge_render_texture_sample_device(crowd.ctx, Int32(slot), deviceUVs, Int32(count), deviceRGBA))
    }
}
