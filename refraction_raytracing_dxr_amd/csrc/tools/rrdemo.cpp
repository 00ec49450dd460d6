// rrdemo -- headless replacement of the reference's WinMain frame pump (WinMain.cpp:37-60):
// initialize once, drawFrame N times, optionally dump frames as binary PPM.
//   rrdemo --mesh shell.obj --env envmap.png [--size 1024x768] [--frames 10] [--out frame_%03d.ppm]
//          [--pump] [--frames-per-dispatch F] [--in-flight L]     (--pump: the loop without per-frame read-back)
//          [--stream]                                              (every frame to host memory, copies overlap rendering)
//          [--spp N]                                               (N = 1, 2, 4, 8, 16 samples per pixel, per-frame path only)
//          [--adaptive BASE:THRESHOLD]                             (with --spp N: BASE samples everywhere, N where contrast exceeds THRESHOLD)
//          [--lens RADIUS:FOCUS]                                   (with --spp N: a thin lens of that aperture radius, sharp at distance FOCUS)
//          [--dispersion BANDS[:ABBE]]                             (with --spp N, default 1: N positions x BANDS bands of the Abbe number, default 30)
//          [--materials "IOR:R,G,B;IOR:R,G,B;..."]                 (with --spp N, default 1: a material table, absorption per unit length; instance i is made of row i modulo the rows)
//          [--nested]                                              (with --materials: the nested-media ray tree, rr_render_nested)
//          [--floor R,G,B[:S]]                                     (with --nested --materials: an opaque floor of that albedo under the mesh, with specular S in every channel; rr_render_surfaces)
//          [--light x,y,z:R,G,B | --light @x,y,z:R,G,B]            (with --nested --materials, up to 8 times: a directional light towards (x, y, z), or with @ a point light at (x, y, z), of that radiance)
//          [--transparent-shadows K]                               (with --floor and --light, 0 <= K <= 16: shadow rays pass glass in at most K steps and take its tint, rr_set_shadow_steps)
//          [--compose]                                             (with --spp N and --materials: --lens, --dispersion and --nested together, rr_render_composed; the Abbe number applies to every row)
//          [--shutter K:DT]                                        (with --compose: every frame over K scene keys spread over DT radians of the orbit, rr_render_shutter; N x K x BANDS <= 64)
//          [--lit [--soft S]]                                      (with --compose, with or without --shutter: --floor and --light through the lens, rr_render_lit; every point light a square of half-edge S in the xz-plane)
//          [--gpus N [--frames-per-gather F]]                      (one process per GPU: tiles, one RCCL gather per F frames)
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <signal.h>
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include "../host/RefractionDemo.hpp"

extern char** environ;

// --gpus N: this process only starts N copies of itself (ranks 0..N-1, device = --device + rank) and waits for them; it never
// touches a GPU.  Rank 0 makes the RCCL id and leaves it in a file the others wait for; the file lives in a directory only this
// user can enter (mkdtemp, mode 0700), so nobody else on the machine can plant it or a link in its place.  When a rank fails
// -- or cannot be started -- the others are ended too: they would wait in RCCL for it for ever.
static int launch_ranks(int argc, char** argv, int gpus)
{
    char dir[] = "/tmp/rrdemo.XXXXXX";
    if (!mkdtemp(dir)) { perror("mkdtemp"); return 1; }
    const std::string idfile = std::string(dir) + "/id";
    std::vector<pid_t> pids;
    bool ok = true;
    for (int r = 0; r < gpus && ok; ++r) {
        std::vector<std::string> a(argv, argv + argc);
        a.push_back("--rank"); a.push_back(std::to_string(r));
        a.push_back("--id-file"); a.push_back(idfile);
        std::vector<char*> av;
        for (auto& x : a) av.push_back(const_cast<char*>(x.c_str()));
        av.push_back(nullptr);
        pid_t pid;
        if (posix_spawn(&pid, "/proc/self/exe", nullptr, nullptr, av.data(), environ) != 0) { fprintf(stderr, "cannot start rank %d\n", r); ok = false; break; }
        pids.push_back(pid);
    }
    size_t left = pids.size();
    std::vector<bool> done(pids.size(), false);
    auto end_the_rest = [&] { for (size_t i = 0; i < pids.size(); ++i) if (!done[i]) kill(pids[i], SIGTERM); };
    if (!ok) end_the_rest();
    while (left > 0) {
        int st = 0;
        const pid_t pid = waitpid(-1, &st, 0);
        if (pid < 0) { ok = false; break; }
        for (size_t i = 0; i < pids.size(); ++i)
            if (pids[i] == pid && !done[i]) {
                done[i] = true; --left;
                if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) { if (ok) end_the_rest(); ok = false; }
            }
    }
    unlink(idfile.c_str());
    unlink((idfile + ".tmp").c_str());
    rmdir(dir);
    return ok ? 0 : 1;
}

int main(int argc, char** argv)
{
    RefractionDemo::Options opt;
    int frames = 1, fpd = 1, in_flight = 2, gpus = 0, rank = -1, fpg = 16, spp = 0, base = 0, n_bands = 0, n_keys = 0;
    float threshold = 0.0f, lens_radius = 0.0f, lens_focus = 0.0f, abbe = 30.0f, shutter_dt = 0.0f;
    bool have_lens = false, pump = false, stream = false, nested = false, compose = false, lit = false, have_soft = false;
    float soft = 0.0f;
    std::vector<rr_material> materials;
    std::vector<rr_light> lights;
    bool have_floor = false;
    float floor_albedo[3] = { 0.0f, 0.0f, 0.0f }, floor_specular = 0.0f;
    bool have_shadow_steps = false;
    int shadow_steps = 0;
    std::string out, idfile;
    for (int i = 1; i < argc; ++i) {
        auto arg = [&](const char* name) { return !strcmp(argv[i], name) && i + 1 < argc; };
        if (arg("--mesh")) opt.mesh_path = argv[++i];
        else if (arg("--env")) opt.env_path = argv[++i];
        else if (arg("--frames")) frames = atoi(argv[++i]);
        else if (arg("--out")) out = argv[++i];
        else if (!strcmp(argv[i], "--pump")) pump = true;
        else if (!strcmp(argv[i], "--stream")) stream = true;
        else if (!strcmp(argv[i], "--nested")) nested = true;
        else if (!strcmp(argv[i], "--compose")) compose = true;
        else if (!strcmp(argv[i], "--lit")) lit = true;
        else if (arg("--soft")) {
            int used = 0;
            if (sscanf(argv[++i], "%f%n", &soft, &used) != 1 || argv[i][used] != 0 || !(soft >= 0.0f) || !std::isfinite(soft)) { fprintf(stderr, "--soft takes S, a finite half-edge >= 0\n"); return 2; }
            have_soft = true;
        }
        else if (arg("--transparent-shadows")) {
            int used = 0;
            if (sscanf(argv[++i], "%d%n", &shadow_steps, &used) != 1 || argv[i][used] != 0 || shadow_steps < 0 || shadow_steps > RR_SHADOW_MAX_STEPS) { fprintf(stderr, "--transparent-shadows takes K, 0 <= K <= 16\n"); return 2; }
            have_shadow_steps = true;
        }
        else if (arg("--frames-per-dispatch")) fpd = atoi(argv[++i]);
        else if (arg("--in-flight")) in_flight = atoi(argv[++i]);
        else if (arg("--spp")) {
            spp = atoi(argv[++i]);
            if (spp != 1 && spp != 2 && spp != 4 && spp != 8 && spp != 16) { fprintf(stderr, "--spp must be 1, 2, 4, 8 or 16\n"); return 2; }
        }
        else if (arg("--adaptive")) {
            if (sscanf(argv[++i], "%d:%f", &base, &threshold) != 2 || base < 1 || !(threshold >= 0.0f)) { fprintf(stderr, "--adaptive takes BASE:THRESHOLD, BASE >= 1, THRESHOLD >= 0\n"); return 2; }
        }
        else if (arg("--lens")) {
            if (sscanf(argv[++i], "%f:%f", &lens_radius, &lens_focus) != 2 || !(lens_radius >= 0.0f) || !(lens_focus > 0.0f)) { fprintf(stderr, "--lens takes RADIUS:FOCUS, RADIUS >= 0, FOCUS > 0\n"); return 2; }
            have_lens = true;
        }
        else if (arg("--dispersion")) {
            const int got = sscanf(argv[++i], "%d:%f", &n_bands, &abbe);
            if (got < 1 || n_bands < 1 || n_bands > 64 || (got == 1 && strchr(argv[i], ':')) || !(abbe > 0.0f)) { fprintf(stderr, "--dispersion takes BANDS[:ABBE], 1 <= BANDS <= 64, ABBE > 0\n"); return 2; }
        }
        else if (arg("--shutter")) {
            if (sscanf(argv[++i], "%d:%f", &n_keys, &shutter_dt) != 2 || n_keys < 1 || n_keys > RR_MAX_SCENE_KEYS || !(shutter_dt >= 0.0f)) { fprintf(stderr, "--shutter takes K:DT, 1 <= K <= 16, DT >= 0\n"); return 2; }
        }
        else if (arg("--materials")) {
            bool ok = true;
            for (const char* q = argv[++i]; ok && *q;) {
                rr_material m;
                int used = 0;
                ok = sscanf(q, "%f:%f,%f,%f%n", &m.ior, &m.sigma_a[0], &m.sigma_a[1], &m.sigma_a[2], &used) == 4 && (q[used] == ';' || q[used] == 0) &&
                     m.ior > 0.0f && m.sigma_a[0] >= 0.0f && m.sigma_a[1] >= 0.0f && m.sigma_a[2] >= 0.0f;
                materials.push_back(m);
                q += used + (q[used] == ';' ? 1 : 0);
            }
            if (!ok || materials.empty()) { fprintf(stderr, "--materials takes IOR:R,G,B rows separated by ';', IOR > 0, R, G, B >= 0\n"); return 2; }
        }
        else if (arg("--floor")) {
            int used = 0;
            const char* q = argv[++i];
            bool ok = sscanf(q, "%f,%f,%f%n", &floor_albedo[0], &floor_albedo[1], &floor_albedo[2], &used) == 3 && (q[used] == ':' || q[used] == 0);
            if (ok && q[used] == ':') { int more = 0; ok = sscanf(q + used + 1, "%f%n", &floor_specular, &more) == 1 && q[used + 1 + more] == 0; }
            if (!ok || !(floor_albedo[0] >= 0.0f) || !(floor_albedo[1] >= 0.0f) || !(floor_albedo[2] >= 0.0f) || !(floor_specular >= 0.0f)) { fprintf(stderr, "--floor takes R,G,B[:S], all >= 0\n"); return 2; }
            have_floor = true;
        }
        else if (arg("--light")) {
            const char* q = argv[++i];
            const bool point = q[0] == '@';
            double v[3];
            rr_light l;
            int used = 0;
            memset(&l, 0, sizeof l);
            if (sscanf(q + (point ? 1 : 0), "%lf,%lf,%lf:%f,%f,%f%n", &v[0], &v[1], &v[2], &l.radiance[0], &l.radiance[1], &l.radiance[2], &used) != 6 || q[(point ? 1 : 0) + used] != 0) { fprintf(stderr, "--light takes x,y,z:R,G,B, or @x,y,z:R,G,B for a point light\n"); return 2; }
            const double xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];       // one operation per statement: nothing to fuse
            const double xy = xx + yy;
            const double sum = xy + zz;
            const double len = sqrt(sum);
            if (!point && !(len > 0.0 && std::isfinite(len))) { fprintf(stderr, "--light: a direction must not be zero\n"); return 2; }
            for (int c = 0; c < 3; ++c) l.v[c] = (float)(point ? v[c] : v[c] / len);      // a direction is normalised in double, then rounded
            l.kind = point ? RR_LIGHT_POINT : RR_LIGHT_DIRECTIONAL;
            l.shadow_mask = 0xffu;
            if (lights.size() == RR_MAX_LIGHTS) { fprintf(stderr, "--light: at most 8 lights\n"); return 2; }
            lights.push_back(l);
        }
        else if (arg("--device")) opt.device = atoi(argv[++i]);
        else if (arg("--gpus")) gpus = atoi(argv[++i]);
        else if (arg("--frames-per-gather")) fpg = atoi(argv[++i]);
        else if (arg("--rank")) rank = atoi(argv[++i]);
        else if (arg("--id-file")) idfile = argv[++i];
        else if (!strcmp(argv[i], "--tonemap")) opt.dispatch.flags |= RR_DISPATCH_TONEMAP_REINHARD;      // c / (1 + c) before the UNORM8 store
        else if (arg("--max-refract")) opt.dispatch.max_refract = atoi(argv[++i]);
        else if (arg("--max-reflect")) opt.dispatch.max_reflect = atoi(argv[++i]);
        else if (arg("--size")) { if (sscanf(argv[++i], "%dx%d", &opt.width, &opt.height) != 2) { fprintf(stderr, "bad --size\n"); return 2; } }
        else { fprintf(stderr, "usage: rrdemo --mesh M.obj --env E.(hdr|png) [--size WxH] [--frames N] [--out f_%%03d.ppm] [--spp N [--adaptive BASE:THRESHOLD | --lens RADIUS:FOCUS]] [--dispersion BANDS[:ABBE]] [--materials IOR:R,G,B;... [--nested [--floor R,G,B[:S]] [--light [@]x,y,z:R,G,B]... [--transparent-shadows K]]] [--compose [--shutter K:DT] [--lit [--floor R,G,B[:S]] [--light [@]x,y,z:R,G,B]... [--soft S]]]\n"); return 2; }
    }
    if (spp && (stream || pump || gpus > 0)) { fprintf(stderr, "--spp renders frame by frame: it cannot be combined with --stream, --pump or --gpus\n"); return 2; }
    if (compose) {          // the frames that refuse each other below, in one call: a lens and dispersion on the nested-media tree
        if (!spp || materials.empty()) { fprintf(stderr, "--compose needs --spp N and --materials\n"); return 2; }
        if (base || pump) { fprintf(stderr, "--compose cannot be combined with --adaptive or --pump\n"); return 2; }
        if ((long long)spp * (n_bands ? n_bands : 1) > 64) { fprintf(stderr, "--compose: --spp N times BANDS must not exceed 64 samples\n"); return 2; }
        if ((long long)spp * (n_keys ? n_keys : 1) * (n_bands ? n_bands : 1) > 64) { fprintf(stderr, "--shutter: --spp N times K times BANDS must not exceed 64 samples\n"); return 2; }
    }
    if (n_keys && !compose) { fprintf(stderr, "--shutter K:DT needs --compose\n"); return 2; }
    if (base && (!spp || base > spp)) { fprintf(stderr, "--adaptive BASE:THRESHOLD needs --spp N with BASE <= N\n"); return 2; }
    if (have_lens && (!spp || base)) { fprintf(stderr, "--lens RADIUS:FOCUS needs --spp N and cannot be combined with --adaptive\n"); return 2; }
    if (n_bands) {
        if (!compose && (base || have_lens)) { fprintf(stderr, "--dispersion BANDS[:ABBE] cannot be combined with --adaptive or --lens\n"); return 2; }
        if (stream || pump || gpus > 0) { fprintf(stderr, "--dispersion renders frame by frame: it cannot be combined with --stream, --pump or --gpus\n"); return 2; }
        if (!spp) spp = 1;
        if (spp < 0 || (long long)spp * n_bands > 64) { fprintf(stderr, "--dispersion: --spp N times BANDS must not exceed 64 samples\n"); return 2; }
    }
    if (!materials.empty()) {
        if (!compose && (base || have_lens || n_bands)) { fprintf(stderr, "--materials cannot be combined with --adaptive, --lens or --dispersion\n"); return 2; }
        if (stream || pump || gpus > 0) { fprintf(stderr, "--materials renders frame by frame: it cannot be combined with --stream, --pump or --gpus\n"); return 2; }
        if (!spp) spp = 1;
    }
    if (nested && materials.empty()) { fprintf(stderr, "--nested needs --materials\n"); return 2; }
    const bool surfaces = have_floor || !lights.empty();
    if (lit && !compose) { fprintf(stderr, "--lit needs --compose\n"); return 2; }
    if (have_soft && !lit) { fprintf(stderr, "--soft S needs --lit\n"); return 2; }
    if (surfaces && !lit && (!nested || materials.empty())) { fprintf(stderr, "--floor and --light need --nested --materials\n"); return 2; }
    if (surfaces && !lit && (compose || n_keys || base || have_lens || n_bands)) { fprintf(stderr, "--floor and --light render with the nested tree alone: they cannot be combined with --compose, --shutter, --adaptive, --lens or --dispersion\n"); return 2; }
    if (!lights.empty() && !have_floor) { fprintf(stderr, "--light needs --floor: glass is not lit by lights\n"); return 2; }
    if (have_shadow_steps && (!have_floor || lights.empty())) { fprintf(stderr, "--transparent-shadows K needs --floor and --light: a shadow falls on the floor, from a light\n"); return 2; }
    if (gpus > 0 && rank < 0) return launch_ranks(argc, argv, gpus);
    if (gpus > 0) {         // one rank of a sharded run
        unsigned char id[128];
        const std::string tmp = idfile + ".tmp";
        if (rank == 0) {
            if (rr_comm_unique_id(id) != RR_OK) { fprintf(stderr, "rr_comm_unique_id failed (is librccl.so installed?)\n"); return 1; }
            FILE* f = fopen(tmp.c_str(), "wb");
            if (!f || fwrite(id, 1, sizeof id, f) != sizeof id) { fprintf(stderr, "cannot write %s\n", tmp.c_str()); return 1; }
            fclose(f);
            rename(tmp.c_str(), idfile.c_str());
        } else {
            FILE* f = nullptr;
            for (int tries = 0; tries < 6000 && !(f = fopen(idfile.c_str(), "rb")); ++tries) usleep(10000);
            if (!f || fread(id, 1, sizeof id, f) != sizeof id) { fprintf(stderr, "rank %d: no RCCL id from rank 0\n", rank); return 1; }
            fclose(f);
        }
        opt.device += rank;
        int rc = RefractionDemo::initializeSharded(opt, rank, gpus, id);
        if (rc != RR_OK) { fprintf(stderr, "rank %d: initialize failed (%d): %s\n", rank, rc, RefractionDemo::lastError()); return 1; }
        auto t0 = std::chrono::steady_clock::now();
        rr_stats st;
        if ((rc = RefractionDemo::pumpSharded(frames, fpg, &st)) != RR_OK) { fprintf(stderr, "rank %d: pump failed (%d): %s\n", rank, rc, RefractionDemo::lastError()); return 1; }
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("rank %d of %d: %d frames of %dx%d in %.3f s (%.1f fps; %.1f Mrays/s on this rank; %d frames per gather)\n", rank, gpus, frames,
               opt.width, opt.height, s, frames / s, (double)st.rays / s / 1e6, fpg);
        if (rank == 0 && !out.empty()) {
            char name[1024];
            snprintf(name, sizeof name, out.c_str(), frames - 1);
            FILE* f = fopen(name, "wb");
            if (!f) { fprintf(stderr, "cannot write %s\n", name); return 1; }
            fprintf(f, "P6\n%d %d\n255\n", opt.width, opt.height);
            const auto& bb = RefractionDemo::backBuffer();
            for (size_t p = 0; p < (size_t)opt.width * opt.height; ++p) fwrite(&bb[p * 4], 1, 3, f);
            fclose(f);
        }
        RefractionDemo::shutdown();
        return 0;
    }
    int rc = RefractionDemo::initialize(opt);
    if (rc != RR_OK) { fprintf(stderr, "initialize failed (%d): %s\n", rc, RefractionDemo::lastError()); return 1; }
    if (!materials.empty() && (rc = RefractionDemo::setMaterials(materials.data(), (int)materials.size())) != RR_OK) {
        fprintf(stderr, "setMaterials failed (%d): %s\n", rc, RefractionDemo::lastError());
        return 1;
    }
    if (have_floor && (rc = RefractionDemo::setFloorAndLights(floor_albedo, floor_specular, lights.data(), (int)lights.size())) != RR_OK) {
        fprintf(stderr, "setFloorAndLights failed (%d): %s\n", rc, RefractionDemo::lastError());
        return 1;
    }
    if (have_shadow_steps && (rc = rr_set_shadow_steps(RefractionDemo::context(), (uint32_t)shadow_steps)) != RR_OK) {
        fprintf(stderr, "rr_set_shadow_steps failed (%d): %s\n", rc, rr_last_error(RefractionDemo::context()));
        return 1;
    }
    if (have_soft && (rc = RefractionDemo::setLightSoftness(soft)) != RR_OK) {
        fprintf(stderr, "setLightSoftness failed (%d): %s\n", rc, RefractionDemo::lastError());
        return 1;
    }
    auto t0 = std::chrono::steady_clock::now();
    if (pump) {
        rr_stats st;
        if ((rc = RefractionDemo::pump(frames, fpd, in_flight, &st)) != RR_OK) { fprintf(stderr, "pump failed (%d): %s\n", rc, RefractionDemo::lastError()); return 1; }
        double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("%d frames of %dx%d in %.3f s (%.1f fps, %.1f Mrays/s; %d per dispatch, %d in flight)\n", frames, opt.width, opt.height, s,
               frames / s, (double)st.rays / s / 1e6, fpd, in_flight);
        if (!out.empty()) {                              // the frame the loop ended on
            char name[1024];
            snprintf(name, sizeof name, out.c_str(), frames - 1);
            FILE* f = fopen(name, "wb");
            if (!f) { fprintf(stderr, "cannot write %s\n", name); return 1; }
            fprintf(f, "P6\n%d %d\n255\n", opt.width, opt.height);
            const auto& bb = RefractionDemo::backBuffer();
            for (size_t p = 0; p < (size_t)opt.width * opt.height; ++p) fwrite(&bb[p * 4], 1, 3, f);
            fclose(f);
        }
        frames = 0;
    }
    if (stream && frames > 0) {
        // chunks of up to 64 frames through one page-locked host buffer; --out writes every frame of every chunk
        const size_t fb = (size_t)opt.width * opt.height * 4;
        const int chunk = frames < 64 ? frames : 64;
        std::vector<uint8_t> host((size_t)chunk * fb);
        const bool pinned = rr_host_register(RefractionDemo::context(), host.data(), host.size()) == RR_OK;
        t0 = std::chrono::steady_clock::now();                      // page-locking the buffer is set-up, not frame time
        double first_chunk_s = 0.0;
        for (int k0 = 0; k0 < frames; k0 += chunk) {
            const int n = frames - k0 < chunk ? frames - k0 : chunk;
            if (k0 == chunk) first_chunk_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if ((rc = RefractionDemo::stream(n, fpd, in_flight, host.data())) != RR_OK) { fprintf(stderr, "stream failed (%d): %s\n", rc, RefractionDemo::lastError()); return 1; }
            for (int k = 0; k < n && !out.empty(); ++k) {
                char name[1024];
                snprintf(name, sizeof name, out.c_str(), k0 + k);
                FILE* f = fopen(name, "wb");
                if (!f) { fprintf(stderr, "cannot write %s\n", name); return 1; }
                fprintf(f, "P6\n%d %d\n255\n", opt.width, opt.height);
                for (size_t p = 0; p < (size_t)opt.width * opt.height; ++p) fwrite(&host[(size_t)k * fb + p * 4], 1, 3, f);
                fclose(f);
            }
        }
        if (pinned) rr_host_unregister(RefractionDemo::context(), host.data());
        double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("%d frames of %dx%d in %.3f s (%.1f fps delivered to %s host memory; %d per dispatch, %d in flight)\n", frames, opt.width,
               opt.height, s, frames / s, pinned ? "page-locked" : "pageable", fpd, in_flight);
        if (first_chunk_s > 0.0 && out.empty())     // the first chunk pays for cold code, streams and first-touch of the host pages
            printf("after the first %d frames: %.1f fps\n", chunk, (frames - chunk) / (s - first_chunk_s));
        frames = 0;
    }
    uint64_t refined = 0;
    for (int k = 0; k < frames; ++k) {
        uint64_t n_ref = 0;
        const rr_lens lens = { lens_radius, lens_focus };
        rc = lit ? RefractionDemo::drawFrameLit(spp, have_lens ? &lens : nullptr, n_bands, abbe, n_keys, shutter_dt) : n_keys ? RefractionDemo::drawFrameShutter(spp, have_lens ? &lens : nullptr, n_bands, abbe, n_keys, shutter_dt) : compose ? RefractionDemo::drawFrameComposed(spp, have_lens ? &lens : nullptr, n_bands, abbe) : have_floor ? RefractionDemo::drawFrameSurfaces(spp) : nested ? RefractionDemo::drawFrameNested(spp) : !materials.empty() ? RefractionDemo::drawFrameMaterials(spp) : base ? RefractionDemo::drawFrameAdaptive(base, spp, threshold, &n_ref) : n_bands ? RefractionDemo::drawFrameSpectral(spp, n_bands, abbe) : have_lens ? RefractionDemo::drawFrameLens(spp, lens_radius, lens_focus) : spp ? RefractionDemo::drawFrameSamples(spp) : RefractionDemo::drawFrame();
        refined += n_ref;
        if (rc != RR_OK) { fprintf(stderr, "drawFrame failed (%d): %s\n", rc, RefractionDemo::lastError()); return 1; }
        if (!out.empty()) {
            char name[1024];
            snprintf(name, sizeof name, out.c_str(), k);
            FILE* f = fopen(name, "wb");
            if (!f) { fprintf(stderr, "cannot write %s\n", name); return 1; }
            fprintf(f, "P6\n%d %d\n255\n", opt.width, opt.height);
            const auto& bb = RefractionDemo::backBuffer();
            for (size_t p = 0; p < (size_t)opt.width * opt.height; ++p) fwrite(&bb[p * 4], 1, 3, f);
            fclose(f);
        }
    }
    double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (frames && lit)
        printf("%d lit frames of %dx%d at %d samples per pixel x %d keys x %d bands with %d materials under %d lights in %.3f s (%.1f fps incl. key captures and readback)\n",
               frames, opt.width, opt.height, spp, n_keys ? n_keys : 1, n_bands ? n_bands : 1, (int)materials.size(), (int)lights.size(), s, frames / s);
    else if (frames && n_keys)
        printf("%d shutter frames of %dx%d at %d samples per pixel x %d keys x %d bands with %d materials in %.3f s (%.1f fps incl. key captures and readback)\n", frames,
               opt.width, opt.height, spp, n_keys, n_bands ? n_bands : 1, (int)materials.size(), s, frames / s);
    else if (frames && compose)
        printf("%d composed frames of %dx%d at %d samples per pixel x %d bands with %d materials in %.3f s (%.1f fps incl. readback)\n", frames, opt.width,
               opt.height, spp, n_bands ? n_bands : 1, (int)materials.size(), s, frames / s);
    else if (frames && base)
        printf("%d frames of %dx%d at %d to %d samples per pixel (threshold %g) in %.3f s (%.1f fps incl. readback); %.2f %% of the pixels refined\n", frames,
               opt.width, opt.height, base, spp, threshold, s, frames / s, 100.0 * (double)refined / ((double)frames * opt.width * opt.height));
    else if (frames && n_bands)
        printf("%d frames of %dx%d at %d samples per pixel x %d bands of Abbe number %g in %.3f s (%.1f fps incl. readback)\n", frames, opt.width,
               opt.height, spp, n_bands, abbe, s, frames / s);
    else if (frames && have_floor)
        printf("%d frames of %dx%d at %d samples per pixel with %d materials (nested media) on a floor under %d lights in %.3f s (%.1f fps incl. readback)\n", frames,
               opt.width, opt.height, spp, (int)materials.size(), (int)lights.size(), s, frames / s);
    else if (frames && !materials.empty())
        printf("%d frames of %dx%d at %d samples per pixel with %d materials%s in %.3f s (%.1f fps incl. readback)\n", frames, opt.width, opt.height, spp,
               (int)materials.size(), nested ? " (nested media)" : "", s, frames / s);
    else if (frames && have_lens)
        printf("%d frames of %dx%d at %d samples per pixel through a lens of radius %g focused at %g in %.3f s (%.1f fps incl. readback)\n", frames, opt.width,
               opt.height, spp, lens_radius, lens_focus, s, frames / s);
    else if (frames && spp) printf("%d frames of %dx%d at %d samples per pixel in %.3f s (%.1f fps incl. readback)\n", frames, opt.width, opt.height, spp, s, frames / s);
    else if (frames) printf("%d frames of %dx%d in %.3f s (%.1f fps incl. readback)\n", frames, opt.width, opt.height, s, frames / s);
    RefractionDemo::shutdown();
    return 0;
}
